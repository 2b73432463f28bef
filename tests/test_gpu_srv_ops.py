"""Every launch of the f16 server networks (BASELINE configs[4], precision "fp16") checked ALONE against a float64 reference of the
op it runs (tools/srv_ref.py), fed the device's own f16 inputs: the error then comes only from that launch's rounding points and
the bound is per element (no tensor-wide tolerance, no compounding over 50 layers).  keep_all runs check every plan op; production
runs check every fused launch (the fused MLP, the head tail, the concat-folded conv) after asserting that its inputs equal the
keep_all run's bit for bit; uploaded hostile inputs check the LayerNorm, attention and GEMM launches at their edges; child processes
check the knobs read once per process (OCR_SRV_MLPLN=1, OCR_SRV_ATTN_PAIR=0).  The six mutations of srv_ref.MUTATIONS must fail."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [("det", (1, 32, 32)), ("det", (2, 96, 160)), ("rec", (1, 48, 320)), ("rec", (7, 48, 320))]
_REFS = {}


def _ref(kind):
    import oracle as O
    import srv_ref
    if kind not in _REFS:
        _REFS[kind] = srv_ref.Ref(O.plan_text("srv_" + kind), O.load_weights("srv_" + kind), half=True)
    return _REFS[kind]


def _srv_ready():
    import synth_weights
    synth_weights.ensure_server(ROOT)


def _fetch_all(net):
    """every tensor of the last run (tid -> f64); t[0] = the packed f16 input (the plan's input as the launches read it)"""
    t = {tid: net.fetch(tid).astype(np.float64) for tid in range(1, net.num_tensors())}
    t[0] = net.fetch(net.num_tensors()).astype(np.float64)
    return t


def _lpr(c):
    """layernorm_h_kernel<LPR> of a width (launch_layernorm): 16 up to 256 channels, 32 up to 512, 64 beyond"""
    return 16 if c // 8 <= 32 else 32 if c // 8 <= 64 else 64


def _worst(res, into):
    for kind, r in res:
        into[kind] = max(into.get(kind, 0.0), r)
    return into


def _report(title, worst):
    print("%s: worst err/bound  %s" % (title, "  ".join("%s %.3f" % kv for kv in sorted(worst.items()))))


def _keep_all_check(kind, shape, seed):
    import srv_ref
    ref = _ref(kind)
    x = np.random.RandomState(seed).randn(*shape, 3).astype(np.float32)
    net = _pkg().SrvNet(kind, "fp16")
    net.forward(x, keep_all=True)
    launches = net.launches()
    t = _fetch_all(net)
    net.close()
    assert np.array_equal(t[0][..., :3], srv_ref.f16(x)), "pack_input"
    res = srv_ref.check_tensors(ref, t)
    return ref, t, launches, res


_PKG = []


def _pkg():
    if not _PKG:
        from __graft_entry__ import load_package
        _PKG.append(load_package())
    return _PKG[0]


@pytest.mark.parametrize("kind,shape", SHAPES)
def test_every_launch_of_a_keep_all_run_within_its_bound(pkg, built, kind, shape):
    """keep_all (every op a launch, every tensor kept): each op's output against the float64 reference evaluated on the device's
    own f16 inputs - finite and within the per-element bound everywhere.  det 1 x 32 x 32: the last stage is one pixel (M below
    every tile); rec 1 line: M = 960 / 480 / 240 (partial 256- and 64-row tiles); rec 7 lines"""
    _srv_ready()
    ref, t, launches, res = _keep_all_check(kind, shape, 100 + shape[0] + shape[2])
    worst = _worst(res.values(), {})
    _report("fp16 %s %s" % (kind, shape), worst)
    bad = {ref.ops[k]["kv"].get("o"): v for k, v in res.items() if not v[1] <= 1.0}
    assert not bad, bad
    # the launch table: one launch per op (plus the input's pack), each writing its op's tensor
    outs = sorted(o for _, o, _ in launches[1:])
    assert outs == sorted(int(op["kv"]["o"]) for op in ref.ops if op["kind"] != "output")


def test_the_checker_rejects_six_mutations_of_device_results(pkg, built):
    """on the device's own inputs and outputs (keep_all runs), the checker must REJECT each mutated reference: the residual left out
    of the last row of the last partial M tile of a linear, the last output column's bias dropped, the local window shifted one column
    at the right grid border, one 8-channel granule of the last tap of a K-ordered 3 x 3 conv, LayerNorm with the unbiased variance.
    (count_include_pad: the plans' average pools are unpadded, the mutation changes nothing there - tests/test_srv_ref.py shows it
    rejected on a padded window.)"""
    import srv_ref
    _srv_ready()
    seen = {}
    for kind, shape in (("rec", (1, 48, 320)), ("det", (2, 96, 160))):
        ref, t, _, _ = _keep_all_check(kind, shape, 7)
        for mut in srv_ref.MUTATIONS:
            op = srv_ref.mutation_site(ref, mut)
            if op is None or mut in seen:
                continue
            ym, bm = ref.op(op, t, mut={mut: True})
            seen[mut] = srv_ref.ratio(t[srv_ref.gi(op, "o")], ym, bm)
    print("mutations: err/bound " + " ".join("%s %.1f" % kv for kv in seen.items()))
    assert set(seen) == set(srv_ref.MUTATIONS) - {"avg_include_pad"}, seen
    assert min(seen.values()) > 1.0, seen


def _fused_check(kind, shape, seed, exact_inputs=True):
    """production binding: every fused launch run alone after the launches before it, on inputs bit-equal to keep_all's
    (exact_inputs=False: an absorbed LayerNorm is another arithmetic than keep_all's, the launches behind the first one read other
    values - then the reference takes the inputs the device holds)"""
    import srv_ref
    ref = _ref(kind)
    x = np.random.RandomState(seed).randn(*shape, 3).astype(np.float32)
    net = _pkg().SrvNet(kind, "fp16")
    net.forward(x, keep_all=True)
    t = _fetch_all(net)
    net.forward(x, keep_all=False)
    launches = net.launches()
    worst, checked = {}, []
    for i, (name, out, ins) in enumerate(launches):
        oi = int(name.split(".")[0]) if name[0].isdigit() else -1
        fused = ".mlp_" in name or ".head_tail_" in name or "_cat[" in name
        if not fused:
            continue
        net.run_launches(0, i)
        t_in = {tid: net.fetch(tid).astype(np.float64) for tid in ins}
        if exact_inputs:
            for tid in ins:
                assert np.array_equal(t_in[tid], t[tid]), (name, tid)  # the arena lifetimes up to this launch
        else:
            t = {**t, **t_in}
        net.run_launches(i, 1)
        got = net.fetch(out).astype(np.float64)
        for tid in ins:  # (its output shares no bytes with its inputs)
            assert np.array_equal(net.fetch(tid).astype(np.float64), t_in[tid]), (name, tid)
        op = ref.ops[oi]
        if ".mlp_ln_" in name:
            y, b = ref.mlp(ref.ops[oi], ref.ops[oi + 1], t[ins[0]], absorbed=ref.ops[oi - 1])
            k = "mlp_ln_%d" % op["W"].shape[0]
        elif ".mlp_" in name:
            y, b = ref.mlp(ref.ops[oi], ref.ops[oi + 1], t[ins[0]])
            k = "mlp_%d" % op["W"].shape[0]
        elif ".head_tail_" in name:
            y, b = ref.head_tail(ref.ops[oi], ref.ops[oi + 1], t[ins[0]])
            k = "head_tail"
        else:
            cat = ref.ops[oi - 1]
            tt = dict(t)
            tt[srv_ref.gi(op, "i")] = ref.op(cat, t)[0]
            y, b = ref.op(op, tt)
            k = "conv3x3_cat"
        r = srv_ref.ratio(got, y, b)
        worst[k] = max(worst.get(k, 0.0), r)
        checked.append(name)
        assert r <= 1.0, (name, r)
    net.close()
    return worst, checked


def test_every_fused_launch_in_production_mode(pkg, built):
    """the fused MLP at C = 192 and 256 (every block), the DB head tail (its 64-channel map rounded to f16 in the reference's bound)
    and the concat-folded 3 x 3 conv, each run alone in the production binding on inputs that equal the keep_all run's bit for bit,
    against the reference of the ops it replaces"""
    _srv_ready()
    worst = {}
    w, names = _fused_check("rec", (1, 48, 320), 21)
    worst.update(w)
    assert sum(".mlp_" in n for n in names) == 12, names
    w, names = _fused_check("det", (2, 96, 160), 22)
    worst.update(w)
    assert sum(".head_tail_" in n for n in names) == 1 and sum("_cat[" in n for n in names) == 1, names
    _report("fused launches", worst)


def _hostile_rows(C, rows, rs):
    """LayerNorm rows: |mean| / sigma in {0, 1, 30, 300} (sigma 1 / 8) and constant rows (variance 0), f16 values"""
    import srv_ref
    x = rs.randn(rows, C) / 8
    for r in range(rows):
        kind = r % 5
        if kind == 4:
            x[r] = rs.choice([-2.0, 0.5, 3.0, 40.0])
        else:
            x[r] += [0.0, 1.0, 30.0, 300.0][kind] / 8 * (1 if r % 2 else -1)
    return srv_ref.f16(x)


def _attn_hostile(op, shape, rs):
    """qkv rows of an attention launch: head 0 all scores equal (q = 0), head 1 one key in seven dominating (|s| ~ 500), rest random"""
    import srv_ref
    heads, hd = srv_ref.gi(op, "heads"), srv_ref.gi(op, "hd")
    n, h, w, c3 = shape
    qkv = rs.randn(n, h * w, 3, heads, hd)
    qkv[:, :, 0, 0] = 0.0
    pat = np.where(rs.rand(hd) < 0.5, -6.0, 6.0)
    qkv[:, :, 0, 1] = pat
    qkv[:, ::7, 1, 1] = pat
    return srv_ref.f16(qkv.reshape(shape))


def _gemm_hostile(op, shape, rs):
    """rows of a linear's input: every third at +-30000 along the sign of a weight column (outputs past the +-65504 clamp), every
    third in the f16 subnormal range along another column's signs (the product of subnormal operands must not vanish)"""
    import srv_ref
    W = op["W"]
    X = rs.randn(int(np.prod(shape[:-1])), shape[-1])
    for r in range(X.shape[0]):
        j = (r * 37) % W.shape[1]
        if r % 3 == 1:
            X[r] = 30000.0 * np.sign(W[:, j])
        elif r % 3 == 2:
            X[r] = rs.uniform(1e-6, 6e-5, W.shape[0]) * np.sign(W[:, j])
    return srv_ref.f16(X.reshape(shape))


def _hostile_check(kind, shape, seed):
    """production binding; one launch at a time on uploaded inputs: every LayerNorm width, the first attention launch of every
    token count, the first linear (clamp and subnormal rows)"""
    import srv_ref
    ref = _ref(kind)
    rs = np.random.RandomState(seed)
    x = rs.randn(*shape, 3).astype(np.float32)
    net = _pkg().SrvNet(kind, "fp16")
    net.forward(x, keep_all=False)
    launches = net.launches()
    worst, seen = {}, set()
    for i, (name, out, ins) in enumerate(launches):
        oi = int(name.split(".")[0]) if name[0].isdigit() else -1
        if oi < 0:
            continue
        op = ref.ops[oi]
        k = op["kind"]
        if k == "ln":
            key = ("ln", net.fetch(ins[0]).shape[-1])
        elif k == "attn":
            key = ("attn", name.split("@")[1].split("[")[0], name[name.index("["):])
        elif k == "linear" and op["res"] is None and op["act"] == "none":
            key = ("linear",)
        else:
            continue
        if key in seen:
            continue
        seen.add(key)
        shp = net.fetch(ins[0]).shape
        if k == "ln":
            u = _hostile_rows(shp[-1], int(np.prod(shp[:-1])), rs).reshape(shp)
        elif k == "attn":
            u = _attn_hostile(op, shp, rs)
        else:
            u = _gemm_hostile(op, shp, rs)
        net.upload(ins[0], u)
        net.run_launches(i, 1)
        got = net.fetch(out).astype(np.float64)
        y, b = ref.op(op, {srv_ref.gi(op, "i"): u})
        r = srv_ref.ratio(got, y, b)
        label = "%s_%s" % (k, "_".join(str(v) for v in key[1:]))
        worst[label] = r
        assert r <= 1.0, (name, r)
    net.close()
    return worst


def test_hostile_inputs_one_launch_at_a_time(pkg, built):
    """uploaded inputs at the edges: LayerNorm rows whose channels share an offset of 0, 1, 30, 300 sigma and constant rows (every
    width: layernorm_h_kernel<16> at C = 192, 256 and <32> at C = 512 - <64> needs C > 512, which no plan has); attention rows
    with all scores equal or one key dominating (every token count); linear outputs past the +-65504 clamp and products of f16
    subnormals"""
    _srv_ready()
    worst = _hostile_check("rec", (2, 48, 320), 31)
    _report("hostile", worst)
    lprs = {_lpr(int(k.split("_")[1])) for k in worst if k.startswith("ln_")}
    assert lprs == {16, 32}, worst
    assert any(k.startswith("linear") for k in worst) and sum(k.startswith("attn") for k in worst) == 3, worst


_CHILD = r"""
import json, sys, numpy as np
sys.path[:0] = [sys.argv[1], sys.argv[1] + "/tools", sys.argv[1] + "/oracle", sys.argv[1] + "/tests"]
import test_gpu_srv_ops as T
mode = sys.argv[2]
out = {}
if mode == "mlpln":
    w, names = T._fused_check("rec", (2, 48, 320), 41, exact_inputs=False)
    out["fused"] = w
    out["names"] = names
    # hostile LayerNorm rows into every absorbed-LN launch's raw sum
    import srv_ref
    ref = T._ref("rec")
    rs = np.random.RandomState(42)
    net = T._pkg().SrvNet("rec", "fp16")
    net.forward(rs.randn(2, 48, 320, 3).astype(np.float32), keep_all=False)
    hw = {}
    for i, (name, o, ins) in enumerate(net.launches()):
        if ".mlp_ln_" not in name:
            continue
        oi = int(name.split(".")[0])
        shp = net.fetch(ins[0]).shape
        u = T._hostile_rows(shp[-1], int(np.prod(shp[:-1])), rs).reshape(shp)
        net.upload(ins[0], u)
        net.run_launches(i, 1)
        y, b = ref.mlp(ref.ops[oi], ref.ops[oi + 1], u, absorbed=ref.ops[oi - 1])
        d = np.abs(net.fetch(o).astype(np.float64) - y) / b
        per = d.reshape(-1, shp[-1]).max(-1)
        for r in range(5):
            hw["%s_%d_rows%d" % ("mlp_ln", shp[-1], r)] = max(hw.get("%s_%d_rows%d" % ("mlp_ln", shp[-1], r), 0.0), float(per[r::5].max()))
    net.close()
    out["hostile"] = hw
else:
    ref, t, launches, res = T._keep_all_check("rec", (2, 48, 320), 43)
    out["worst"] = T._worst([v for k, v in res.items() if ref.ops[k]["kind"] == "attn"], {})
    out["variants"] = sorted({n[n.index("["):] for n, _, _ in launches if ".attn_" in n})
print("CHILD " + json.dumps(out))
"""


def test_knobs_in_child_processes(pkg, built):
    """environment knobs are read once per process: OCR_SRV_MLPLN=1 - the LayerNorm absorbed into every fused MLP, each launch alone
    against the float64 LayerNorm-then-MLP with the absorbed form's own rounding points (raw sum, folded image, statistics in the
    kernel), also on the hostile rows; OCR_SRV_ATTN_PAIR=0 - the only runs of attn_h_kernel<4,1> and of the global <8,1>.
    With the default run's <8,2> / <16,2> / local <8,1> every instantiation the plans reach is checked."""
    _srv_ready()
    procs = {}
    for mode, env in (("mlpln", {"OCR_SRV_MLPLN": "1"}), ("nopair", {"OCR_SRV_ATTN_PAIR": "0"})):
        procs[mode] = subprocess.Popen([sys.executable, "-c", _CHILD, ROOT, mode], env=dict(os.environ, **env), stdout=subprocess.PIPE,
                                       stderr=subprocess.PIPE, text=True)
    res = {}
    for mode, pr in procs.items():
        so, se = pr.communicate(timeout=400)
        assert pr.returncode == 0 and "CHILD " in so, (mode, so[-2000:], se[-3000:])
        res[mode] = json.loads(so[so.index("CHILD ") + 6:].splitlines()[0])
    m = res["mlpln"]
    _report("OCR_SRV_MLPLN=1 fused", m["fused"])
    _report("OCR_SRV_MLPLN=1 hostile rows (offset 0, 1, 30, 300 sigma, constant)", m["hostile"])
    assert sum(".mlp_ln_" in n for n in m["names"]) == 12, m["names"]
    assert max(m["fused"].values()) <= 1.0 and max(m["hostile"].values()) <= 1.0, m
    a = res["nopair"]
    _report("OCR_SRV_ATTN_PAIR=0 attention", a["worst"])
    assert a["variants"] == ["[4x1]", "[8x1]"], a["variants"]
    assert max(a["worst"].values()) <= 1.0, a
    # the default binding's instantiations (checked by the keep_all test above)
    net = pkg.SrvNet("rec", "fp16")
    net.forward(np.zeros((1, 48, 320, 3), np.float32), keep_all=True)
    assert sorted({n[n.index("["):] for n, _, _ in net.launches() if ".attn_" in n}) == ["[16x2]", "[8x1]", "[8x2]"]
    net.close()
