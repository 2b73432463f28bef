"""BASELINE configs[4] on the CPU: the hand-written server plans (NOT reference artifacts: tools/make_server_plans.py), the oracle
ops they add, and an independent float64 torch interpretation of the same plans as a second opinion on the oracle."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANS = os.path.join(ROOT, "cpp-paddle-ocr_amd", "plans")


def test_committed_plans_are_what_the_generator_writes(tmp_path):
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_server_plans", os.path.join(ROOT, "tools", "make_server_plans.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    for P in (m.det_plan(), m.rec_plan()):
        assert P.text() == open(os.path.join(PLANS, P.name + ".plan")).read(), P.name
    # ResNet50-vd: 16 bottlenecks; SVTR-L: 3 + 9 + 9 mixing blocks, ten of them local
    det = open(os.path.join(PLANS, "srv_det.plan")).read()
    rec = open(os.path.join(PLANS, "srv_rec.plan")).read()
    assert det.count("w=res") == 52 and det.count("_branch2c.w ep=") == 16 and det.count("type=avg") == 3 and det.count("addup:") == 3
    assert rec.count("\nattn ") == 21 and rec.count("lh=7 lw=11") == 10 and "cout=6625" in rec
    assert "NOT a reference artifact" in det and "NOT a reference artifact" in rec


def test_erf_of_the_gelu(built):
    """ocr_erff (Abramowitz-Stegun 7.1.26 with the contract's exp): within 5e-7 of the real erf (the formula's own 1.5e-7 plus f32 rounding) - the plans' act:gelu is the
    exact GELU to f32 accuracy"""
    import ctypes as C
    import oracle as O
    L = O.lib()
    if not hasattr(L, "oracle_erff"):
        pytest.skip("oracle built without the probe")
    L.oracle_erff.restype = C.c_float
    L.oracle_erff.argtypes = [C.c_float]
    xs = np.concatenate([np.linspace(-6, 6, 4001), [0.0, -0.0, 1e-8, 30.0, -30.0]]).astype(np.float32)
    err = max(abs(L.oracle_erff(float(x)) - math.erf(float(x))) for x in xs)
    assert err <= 5e-7, err


def _torch_run(plan_text, params, x):
    """float64 torch interpretation of a server plan, op by op, written from the plan grammar alone (tools/srv_ref.py)"""
    import srv_ref
    return srv_ref.torch_run(plan_text, params, x)


@pytest.mark.parametrize("net,shape", [("srv_det", (1, 64, 96)), ("srv_rec", (1, 48, 320))])
def test_oracle_matches_an_independent_torch_interpretation(built, net, shape):
    """the oracle's f32 run of a server plan (the arithmetic the device's f32 twin reproduces bit for bit) against torch float64 on
    the same seeded parameters: every tensor within 2e-4 of its own scale, the output (probability map / CTC logits) within 2e-4"""
    import oracle as O
    x = np.random.RandomState(2).randn(shape[0], shape[1], shape[2], 3).astype(np.float32)
    o = O.OracleNet(net)
    got = o.run(x)
    want, tensors = _torch_run(O.plan_text(net), o.weights, x)
    assert got.shape == want.shape
    assert np.abs(got - want).max() <= 2e-4, float(np.abs(got - want).max())
    worst = 0.0
    for tid, w in tensors.items():
        g = o.tensor(tid)
        assert g.shape == w.shape, (tid, g.shape, w.shape)
        worst = max(worst, float(np.abs(g - w).max() / (np.abs(w).max() + 1e-9)))
    assert worst <= 2e-4, worst


def test_server_weights_are_seeded_and_in_the_pdiparams_format(built):
    import synth_weights
    import oracle as O
    paths = synth_weights.ensure_server(ROOT)
    for kind, p in zip(("det", "rec"), paths):
        table = synth_weights.server_param_table(os.path.join(PLANS, "srv_%s.plan" % kind))
        w = O.load_weights("srv_" + kind)
        assert set(w) == {n for n, _ in table}
        n0, d0 = table[0]
        assert np.array_equal(w[n0], synth_weights.synth_server_tensor(n0, d0))
        assert os.path.getsize(p) > sum(int(np.prod(d)) for _, d in table) * 4
