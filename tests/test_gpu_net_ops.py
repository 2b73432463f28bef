"""Every launch of the mobile networks under precision "fp16" (det / cls / rec: what OCR_WORKER_PRECISION=fp16 serves) checked ALONE
against the float64 reference of the op it runs (tools/net_ref.py), fed the device's own fetched inputs: the error is that launch's
rounding points only and the bound is per element - no quantile, no share of elements, no compounding over sixty layers.
keep_all=1: every op a launch.  keep_all=2: the production launch list, fused groups against the composed reference on their
nearest existing inputs.  keep_all=0: the same output bits out of the liveness-reused arena.  Both ragged forms: each sample equals
the sample alone, bit for bit, and passes the per-op check.  The six mutations of net_ref.MUTATIONS must fail on the device's results.
Only binding.Net's forward / forward_ragged / forward_ragged_images / fetch / exists / num_tensors / timing / timing_report are used."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNIFORM = [("cls", (3, 48, 192)), ("det", (3, 64, 64)), ("det", (2, 96, 160)), ("rec", (1, 48, 320)), ("rec", (5, 48, 136)), ("rec", (2, 28, 192))]
RAG_WIDTHS = (320, 333, 40)
RAG_IMAGES = ((96, 160), (64, 64), (32, 96))
_REFS, _RUNS, _NAMES, _PKG = {}, {}, set(), []


def _pkg():
    if not _PKG:
        from __graft_entry__ import load_package
        _PKG.append(load_package())
    return _PKG[0]


def _ref(kind):
    import net_ref
    import oracle as O
    if kind not in _REFS:
        _REFS[kind] = net_ref.Ref(O.plan_text(kind), O.load_weights(kind), half=True)
    return _REFS[kind]


def _collect(net, x0):
    """every existing tensor of the last run (tid -> f64), t[0] = the f32 input; the launch names go to the coverage set"""
    t = {0: np.asarray(x0, np.float64)} if x0 is not None else {}
    ex = {tid for tid in range(1, net.num_tensors()) if net.exists(tid)}
    for tid in sorted(ex):
        t[tid] = net.fetch(tid).astype(np.float64)
    names = set(net.timing_report())
    _NAMES.update(n.split("@")[0].split(".", 2)[0] + "." + n.split("@")[0].split(".", 2)[2] for n in names)
    return t, ex


def _run(kind, shape, keep, seed=11):
    """one uniform fp16 forward, computed once and shared (never modified): (tensors, exists, output)"""
    key = (kind, shape, keep, seed)
    if key not in _RUNS:
        x = np.random.RandomState(seed).randn(shape[0], shape[1], shape[2], 3).astype(np.float32)
        net = _pkg().Net(kind, precision="fp16")
        net.timing(True)
        y = net.forward(x, keep_all=keep)
        t, ex = _collect(net, x) if keep else ({}, set())
        net.close()
        _RUNS[key] = (t, ex, y)
    return _RUNS[key]


def _worst(res):
    w = {}
    for k, r, _ in res.values():
        w[k] = max(w.get(k, 0.0), r)
    return w


def _report(title, worst):
    print("%s: worst err/bound  %s" % (title, "  ".join("%s %.3f" % kv for kv in sorted(worst.items()))))


def _check(kind, t, ex, keep):
    import net_ref
    ref = _ref(kind)
    res = net_ref.check_tensors(ref, t, exists=(lambda i: i in ex) if keep == 2 else None)
    return ref, res


@pytest.mark.parametrize("kind,shape", UNIFORM)
def test_every_launch_of_a_keep_all_run_within_its_bound(pkg, built, kind, shape):
    """keep_all=1: every op is a launch and every tensor is kept; each against Ref.op on the device's own inputs - finite, within the
    per-element bound everywhere, exact ops bit for bit.  Shapes: maps that are no multiple of the 8 x 16 / 4 x 16 tiles, single
    row pairs, last stages of 2 x 2 and 1 x 3 pixels, M below every matrix tile, several images (per-image gate rows), the H = 28 pool"""
    t, ex, _ = _run(kind, shape, 1)
    ref, res = _check(kind, t, ex, 1)
    _report("fp16 keep_all=1 %s %s" % (kind, shape), _worst(res))
    assert len(res) == len(ref.ops) - 1, sorted(set(range(1, len(ref.ops))) - set(res))
    bad = {tid: v[:2] for tid, v in res.items() if not v[1] <= 1.0}
    assert not bad, bad


@pytest.mark.parametrize("kind,shape", UNIFORM)
def test_production_launch_list_within_its_bounds_and_arena_reuse(pkg, built, kind, shape):
    """keep_all=2: the production launch list, every tensor in its own slot - each existing tensor against the reference of its op,
    fused groups against the composed reference; the fused-away tensors are there (missing >= 8 for det and rec, as the fp32 test
    expects); a fusion whose rounding points net_ref states identical (FUSIONS) equals the keep_all=1 tensor bit for bit where its
    inputs do; and
    keep_all=0 (liveness-reused arena in f16 storage) gives the same output bits"""
    import net_ref
    t, ex, y2 = _run(kind, shape, 2)
    ref, res = _check(kind, t, ex, 2)
    _report("fp16 keep_all=2 %s %s" % (kind, shape), _worst(res))
    bad = {tid: v[:2] for tid, v in res.items() if not v[1] <= 1.0}
    assert not bad, bad
    missing = len(ref.ops) - 1 - len(ex)
    if kind in ("det", "rec"):
        assert missing >= 8, missing
    t1 = _run(kind, shape, 1)[0]
    same = [tid for tid, (_, _, met) in res.items() if met and all(net_ref.FUSIONS[m] for m in met)]
    for tid in same:  # (same bits need the same input bits: det's neck feeds this conv from the RSE blocks, fused here and not there)
        ins = ref.by_out[net_ref.gi(ref.by_out[tid], "i")]["ins"]
        if all(np.array_equal(t[i], t1[i]) for i in ins):
            assert np.array_equal(t[tid], t1[tid]), tid
    if kind == "det":
        assert same, "the concat-folded conv ran"
    y0 = _run(kind, shape, 0)[2]
    assert y0.shape == y2.shape and np.array_equal(y0, y2)


def _shapes(ref, h, w):
    """(h, w) of every tensor of one sample (the plan's geometry; C++ truncating division)"""
    import net_ref
    gi = net_ref.gi
    s = {0: (h, w)}
    div = lambda a, b: int(a / b)
    for op in ref.ops:
        k = op["kind"]
        if k == "output":
            continue
        ih, iw = s[op["ins"][-1] if k == "concat" else gi(op, "i")]
        if k in ("conv", "dw", "pool"):
            ph, pw = gi(op, "ph"), gi(op, "pw")
            s[gi(op, "o")] = (div(ih + 2 * ph - gi(op, "kh"), gi(op, "sh")) + 1, div(iw + 2 * pw - gi(op, "kw"), gi(op, "sw")) + 1)
        elif k == "deconv":
            s[gi(op, "o")] = (2 * ih, 2 * iw)
        elif k in ("gap", "sefc"):
            s[gi(op, "o")] = (1, 1)
        elif k == "concat":
            s[gi(op, "o")] = (ih * op["ups"][-1], iw * op["ups"][-1])
        else:
            s[gi(op, "o")] = (ih, iw)
    return s


def _ragged_check(kind, samples, forward):
    """the ragged batch at keep_all 2: every existing tensor, split by sample, equals the sample alone (where that run has it) and
    passes the per-op check; keep_all 0 gives the same output"""
    import net_ref
    ref = _ref(kind)
    net = _pkg().Net(kind, precision="fp16")
    net.timing(True)
    y2 = forward(net, samples, 2)
    tr, ex = _collect(net, None)
    y0 = forward(net, samples, 0)
    assert np.array_equal(y0, y2)
    worst, compared = {}, 0
    offs = {tid: 0 for tid in tr}
    for i, smp in enumerate(samples):
        sh = _shapes(ref, smp.shape[0], smp.shape[1])
        t = {0: smp[None].astype(np.float64)}
        for tid, a in tr.items():
            c = a.shape[-1]
            hw = sh[tid][0] * sh[tid][1]
            flat = a.reshape(-1, c)
            t[tid] = flat[offs[tid]:offs[tid] + hw].reshape(1, sh[tid][0], sh[tid][1], c)
            assert t[tid].size == hw * c, (tid, a.shape, sh[tid])
            offs[tid] += hw
        alone = net.forward(smp[None], keep_all=2)
        assert np.array_equal(alone.reshape(-1), t[ref.out_tid].reshape(-1)), i
        for tid in sorted(ex):
            if net.exists(tid):
                assert np.array_equal(net.fetch(tid).astype(np.float64), t[tid]), (i, tid)
                compared += 1
        res = net_ref.check_tensors(ref, t, exists=lambda j: j in ex)
        bad = {tid: v[:2] for tid, v in res.items() if not v[1] <= 1.0}
        assert not bad, (i, bad)
        for k, r in _worst(res).items():
            worst[k] = max(worst.get(k, 0.0), r)
    for tid, a in tr.items():
        assert offs[tid] == a.reshape(-1, a.shape[-1]).shape[0], tid
    net.close()
    assert compared >= 40 * len(samples)
    return worst


def test_ragged_rec_lines_equal_each_line_alone_and_pass_the_per_op_check(pkg, built):
    """widths 320, 333 (odd at every level), 40 (narrower than a tile row's worth at the low levels) at height 48"""
    rs = np.random.RandomState(21)
    lines = [rs.randn(48, w, 3).astype(np.float32) for w in RAG_WIDTHS]
    _report("fp16 ragged rec", _ragged_check("rec", lines, lambda n, s, k: n.forward_ragged(s, keep_all=k)))


def test_ragged_det_images_equal_each_image_alone_and_pass_the_per_op_check(pkg, built):
    """images 96 x 160, 64 x 64, 32 x 96 in one launch list"""
    rs = np.random.RandomState(22)
    imgs = [rs.randn(h, w, 3).astype(np.float32) for h, w in RAG_IMAGES]
    _report("fp16 ragged det", _ragged_check("det", imgs, lambda n, s, k: n.forward_ragged_images(s, keep_all=k)))


def test_the_checker_rejects_six_mutations_of_device_results(pkg, built):
    """on the device's own inputs and outputs (keep_all=1: rec 5 x 48 x 136, det 2 x 96 x 160, and rec 2 x 28 x 192 for the truncated
    pool window, which no 48-row input has) each mutated reference is rejected with err / bound > 1"""
    import net_ref
    seen = {}
    for kind, shape in (("rec", (5, 48, 136)), ("det", (2, 96, 160)), ("rec", (2, 28, 192))):
        t = _run(kind, shape, 1)[0]
        ref = _ref(kind)
        for mut in net_ref.MUTATIONS:
            op = net_ref.mutation_site(ref, mut, t)
            if op is None or mut in seen:
                continue
            seen[mut] = net_ref.ratio(t[net_ref.gi(op, "o")], *ref.op(op, t, mut={mut: True}))
    print("mutations: err/bound " + " ".join("%s %.3g" % kv for kv in seen.items()))
    assert set(seen) == set(net_ref.MUTATIONS), seen
    assert min(seen.values()) > 1.0, seen


# launch names of the timing report (net.hip names a launch after its op and its fused form, not after the kernel template) ->
# the f16 launcher family behind them.  Which kernel a conv1x1 / conv3x3 / dw5x5 name runs is the binder's choice by shape
# (Net::dense_closure, emit_dw); tests/golden/net_launch_lists.json pins those choices' inputs, the names below pin the routes.
FAMILIES = {
    "stem": "stem3x3_", "direct conv (conv_mfma, one pixel tile per wave)": "conv1x1_", "gated conv (conv_mfma / mt2 / mt16, GATE)": "_gated",
    "conv3x3_tile16": "conv3x3_96_24", "concat folded into conv3x3_tile16": "_cat4", "row-sum conv": "_rowsum", "multi-tap direct conv": "conv1x3_",
    "dw": "dw3x3_", "dw 5x5 (dw_lds on the low maps)": "dw5x5_", "dwpw": "dwpw", "ew": "ew_", "gap": "gap_", "sefc": "sefc_", "concat": "concat_",
    "pool": "pool_", "ln": "ln_", "attn": "attn_", "linear": "linear1x1_", "softmax": "softmax_", "deconv": "deconv1x1_", "det tail": "det_tail",
    "DB head": "db_head_",
}


def test_every_f16_launcher_family_ran(pkg, built):
    """from the timing reports of this file's own runs: every launch route of the fp16 mode ran at least once - a binder change that
    routes around a kernel fails here.  Not visible in a report: the two-pixel-tile (mt2), 32x32x16 (mt16) and LDS depthwise
    kernels share their op's launch name with the plain ones (det 2 x 96 x 160 and rec 5 x 48 x 136 are below mt2's 1024-workgroup
    threshold; the switch test's OCR_CONV_MT2=force child runs it); the fused CTC head and softmax_argmax are bound to the Rec
    stage handle's (arg max, probability) outputs, which binding.Net does not have."""
    for kind, shape in UNIFORM:
        _run(kind, shape, 1)
        _run(kind, shape, 2)
    missing = {fam: pat for fam, pat in FAMILIES.items() if not any(pat in n for n in _NAMES)}
    assert not missing, (missing, sorted(_NAMES))


_SWITCHES = [{"OCR_MFMA_X16": "0"}, {"OCR_FUSE_GAP_MIN": "1", "OCR_CONV_MT2": "force"}, {"OCR_DW_LDS": "0"}, {"OCR_DWPW_ITEMS": "7"},
             {"OCR_DWPW_ITEMS": "1"}, {"OCR_DWPW_FORCE_UPW": "3"}, {"OCR_FUSE": "0"}]
_CHILD = r"""
import json, sys
sys.path[:0] = [sys.argv[1], sys.argv[1] + "/tools", sys.argv[1] + "/oracle", sys.argv[1] + "/tests"]
import test_gpu_net_ops as T
out = {}
for kind, shape in (("det", (2, 96, 160)), ("rec", (5, 48, 136))):
    t, ex, _ = T._run(kind, shape, 2)
    ref, res = T._check(kind, t, ex, 2)
    out[kind] = dict(worst=T._worst(res), bad={str(k): v[:2] for k, v in res.items() if not v[1] <= 1.0}, missing=len(ref.ops) - 1 - len(ex))
print("CHILD " + json.dumps(out))
"""
_SW_RESULTS = {}


def _switch_runs():
    pending, running = list(enumerate(_SWITCHES)), []
    while pending or running:
        while pending and len(running) < 4:
            i, env = pending.pop(0)
            running.append((i, subprocess.Popen([sys.executable, "-c", _CHILD, ROOT], env=dict(os.environ, **env), stdout=subprocess.PIPE,
                                                stderr=subprocess.PIPE, text=True)))
        i, pr = running.pop(0)
        try:
            so, se = pr.communicate(timeout=600)
        except subprocess.TimeoutExpired:
            pr.kill()
            so, se = pr.communicate()
            se += "\nTIMEOUT"
        _SW_RESULTS[i] = (pr.returncode, so, se)


@pytest.mark.parametrize("idx", range(len(_SWITCHES)), ids=["-".join("%s=%s" % kv for kv in e.items()) for e in _SWITCHES])
def test_switches_keep_every_launch_within_its_bound(built, idx):
    """switches are read once per process: child processes, four at a time, each the keep_all=2 check at det 2 x 96 x 160 and
    rec 5 x 48 x 136 - the 32x32x8 forms, the row-sum depthwise path and two pixel tiles per wave on small maps, the register-patch
    5x5 depthwise kernel, odd / single-item / multi-unit pipelines of the fused block, and the unfused list"""
    if not _SW_RESULTS:
        _switch_runs()
    rc, so, se = _SW_RESULTS[idx]
    assert rc == 0 and "CHILD " in so, (so[-2000:], se[-3000:])
    res = json.loads(so[so.index("CHILD ") + 6:].splitlines()[0])
    for kind, r in res.items():
        _report("%s %s" % (_SWITCHES[idx], kind), r["worst"])
        assert not r["bad"], (kind, r["bad"])
        assert (r["missing"] == 0) == (_SWITCHES[idx].get("OCR_FUSE") == "0"), (kind, r["missing"])
