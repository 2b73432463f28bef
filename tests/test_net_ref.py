"""tools/net_ref.py on the CPU: the per-op float64 reference of the mobile plans (det / cls / rec) against the oracle's own tensors
with the fp32 contract's weights (the fold restatement, the absorption, the geometry and the quirks are right before a GPU is
involved), the checker's power (six small local errors are rejected), and the emulated fp16 mode against the tolerances
tests/test_gpu_round4.py states for the device.  The GPU side of the same checker: tests/test_gpu_net_ops.py."""
import numpy as np
import pytest

CASES = [("cls", (2, 48, 192)), ("det", (1, 64, 96)), ("rec", (2, 48, 136)), ("rec", (1, 28, 192))]
_RUNS = {}


def _oracle_run(kind, shape, seed=3):
    """(reference with the f32 weights, the oracle's tensors tid -> f64) - computed once per case, shared, never modified"""
    import net_ref
    import oracle as O
    key = (kind, shape, seed)
    if key not in _RUNS:
        x = np.random.RandomState(seed).randn(shape[0], shape[1], shape[2], 3).astype(np.float32)
        o = O.OracleNet(kind)
        o.run(x)
        ref = net_ref.Ref(O.plan_text(kind), o.weights, half=False)
        t = {0: x.astype(np.float64)}
        for op in ref.ops:
            if op["kind"] != "output":
                t[net_ref.gi(op, "o")] = o.tensor(net_ref.gi(op, "o")).astype(np.float64)
        _RUNS[key] = (ref, t)
    return _RUNS[key]


def test_ocr_expf_is_within_the_constant_the_bounds_take(built):
    """net_ref.EXP_REL (4 u32) against the oracle's ocr_expf over the arguments the networks give it"""
    import net_ref
    import oracle as O
    xs = np.concatenate([np.linspace(-87.0, 20.0, 20001), np.linspace(-1.0, 1.0, 4001)]).astype(np.float32)
    got = np.array([O.lib().oracle_expf(float(v)) for v in xs], np.float64)
    want = np.exp(xs.astype(np.float64))
    assert (np.abs(got - want) / want).max() <= net_ref.EXP_REL


@pytest.mark.parametrize("kind,shape", CASES)
def test_per_op_reference_reproduces_every_oracle_tensor(built, kind, shape):
    """half=False, op by op on the oracle's own inputs: every oracle tensor within the f32 form of the op's bound at every element
    (u32 where the f16 build has u16, no weight rounding); exact ops equal"""
    import net_ref
    ref, t = _oracle_run(kind, shape)
    res = net_ref.check_tensors(ref, t)
    worst = {}
    for tid, (k, r, _) in res.items():
        worst[k] = max(worst.get(k, 0.0), r)
    print(kind, shape, " ".join("%s %.3f" % kv for kv in sorted(worst.items())))
    assert len(res) == len(ref.ops) - 1
    bad = {tid: v[:2] for tid, v in res.items() if not v[1] <= 1.0}
    assert not bad, bad


@pytest.mark.parametrize("kind,shape", CASES)
def test_composed_reference_of_the_fused_groups_on_the_oracles_tensors(built, kind, shape):
    """Ref.composed at half=False with the tensors hidden that the production list of the fp16 mode never writes (the `exists`
    strings tests/golden/net_launch_lists.json records for its fp16 keep_all=2 cases): every remaining oracle tensor within the
    composed bound - the missing tensor evaluated in float64, its error carried through the reader (the din plumbing, the
    w16=False / rounded=False paths, the gate, dwpw, db_head and rowsum groups all run here); each fusion kind is met"""
    import json
    import os
    import net_ref
    gold = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "net_launch_lists.json")))["cases"]
    mask = gold[{"cls": "cls-3x48x192-fp16-keep2", "det": "det-2x96x160-fp16-keep2", "rec": "rec-3x48x320-fp16-keep2"}[kind]]["exists"]
    ref, t = _oracle_run(kind, shape)
    ex = {i for i, c in enumerate(mask) if c == "1"}
    assert len(ex) < len(ref.ops) - 1
    seen = {i: v for i, v in t.items() if i == 0 or i in ex}
    res = net_ref.check_tensors(ref, seen, exists=lambda i: i in ex)
    worst, met = {}, set()
    for tid, (k, r, m) in res.items():
        worst[k] = max(worst.get(k, 0.0), r)
        met |= set(m)
    print(kind, shape, " ".join("%s %.3f" % kv for kv in sorted(worst.items()) if ":" in kv[0]))
    assert len(res) == len(ex)
    bad = {tid: v[:2] for tid, v in res.items() if not v[1] <= 1.0}
    assert not bad, bad
    assert met == {"cls": {"gate"}, "det": {"gate", "dwpw", "db_head", "cat", "rowsum"}, "rec": {"gate", "dwpw"}}[kind], met  # (rowsum: the RSE blocks)


def test_six_mutations_are_rejected_on_the_oracles_tensors(built):
    """each mutation at its site: err / bound > 1 on the oracle's tensors, the unmutated reference <= 1 on the same tensors.  The
    first site per mutation over the cases is taken; drop_last_bias takes a conv whose last folded bias is at least 0.02 in
    magnitude (net_ref.mutation_site) - a channel whose bias is (nearly) zero does not change when it is dropped"""
    import net_ref
    seen = {}
    for kind, shape in CASES:
        ref, t = _oracle_run(kind, shape)
        for mut in net_ref.MUTATIONS:
            op = net_ref.mutation_site(ref, mut, t)
            if op is None or mut in seen:
                continue
            o = net_ref.gi(op, "o")
            good = net_ref.ratio(t[o], *ref.op(op, t))
            bad = net_ref.ratio(t[o], *ref.op(op, t, mut={mut: True}))
            seen[mut] = (kind, o, good, bad)
    print("mutations: " + "  ".join("%s %s.%d %.3f -> %.3g" % ((m,) + v) for m, v in seen.items()))
    assert set(seen) == set(net_ref.MUTATIONS), seen
    for m, (_, _, good, bad) in seen.items():
        assert good <= 1.0 < bad, (m, good, bad)


def test_emulated_fp16_run_stays_within_the_devices_tolerances(built):
    """half=True chained over the whole plan, every f16 tensor rounded as the store would: the emulated rounding points describe
    the mode the device implements - the tolerances are those test_fp16_networks_stay_within_tolerance_of_the_f32_contract states
    against the oracle (same inputs)"""
    import net_ref
    import oracle as O
    rs = np.random.RandomState(2)

    def both(kind, shape):
        x = rs.randn(*shape, 3).astype(np.float32)
        o = O.OracleNet(kind)
        want = o.run(x)
        ref = net_ref.Ref(O.plan_text(kind), o.weights, half=True)
        return want, net_ref.run_chain(ref, x)[ref.out_tid]

    want, y = both("cls", (6, 48, 192))
    want, y = want.reshape(6, 2), y.reshape(6, 2)
    assert np.abs(y - want).max() <= 2e-3 and np.array_equal(y.argmax(1), want.argmax(1))
    want, y = both("det", (2, 160, 224))
    d = np.abs(y.reshape(-1) - want.reshape(-1))
    assert d.mean() <= 2e-3 and np.quantile(d, 0.99) <= 1e-2, (d.mean(), np.quantile(d, 0.99), d.max())
    assert ((y > 0.3) == (want > 0.3)).mean() >= 0.995
    want, y = both("rec", (4, 48, 320))
    want, y = want.reshape(-1, 6625), y.reshape(-1, 6625)
    assert np.abs(y - want).max() <= 0.02 * want.max(), (np.abs(y - want).max(), want.max())
    assert (y.argmax(1) == want.argmax(1)).mean() >= 0.95
