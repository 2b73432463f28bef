"""tools/srv_ref.py on the CPU: the per-op float64 reference of the server plans (and its error bounds) against the oracle's own
tensors, and the checker's power - the f16-rounded reference passes it, six small local errors do not.  The GPU side of the same
checker: tests/test_gpu_srv_ops.py."""
import math

import numpy as np
import pytest

SHAPES = {"srv_det": (1, 64, 96), "srv_rec": (1, 48, 320)}


def _oracle(net, seed):
    import oracle as O
    shape = SHAPES[net]
    x = np.random.RandomState(seed).randn(shape[0], shape[1], shape[2], 3).astype(np.float32)
    o = O.OracleNet(net)
    o.run(x)
    return o, x, O.plan_text(net)


@pytest.mark.parametrize("net", sorted(SHAPES))
def test_per_op_reference_reproduces_every_oracle_tensor(built, net):
    """the reference with the weights as the f32 twin holds them, op by op on the oracle's own f32 tensors: every oracle tensor
    within the op's f32-level bound (the restatement of each op - indexing, padding, windows, epilogue order - is right)"""
    import srv_ref
    o, x, plan = _oracle(net, 3)
    ref = srv_ref.Ref(plan, o.weights, half=False)
    t = {0: x.astype(np.float64)}
    for op in ref.ops:
        if op["kind"] != "output":
            t[srv_ref.gi(op, "o")] = o.tensor(srv_ref.gi(op, "o")).astype(np.float64)
    res = srv_ref.check_tensors(ref, t)
    worst = {}
    for k, (kind, r) in res.items():
        worst[kind] = max(worst.get(kind, 0.0), r)
    print(net, " ".join("%s %.3f" % kv for kv in sorted(worst.items())))
    assert max(worst.values()) <= 1.0, worst


def _f16_inputs(net, seed):
    """the oracle's tensors rounded to f16 - stand-ins for a device run's - and the f16-build reference"""
    import srv_ref
    o, x, plan = _oracle(net, seed)
    ref = srv_ref.Ref(plan, o.weights, half=True)
    t = {0: srv_ref.f16(x)}
    for op in ref.ops:
        if op["kind"] != "output":
            tid = srv_ref.gi(op, "o")
            v = o.tensor(tid).astype(np.float64)
            t[tid] = v if tid == ref.out_tid else srv_ref.f16(v)
    return ref, t


def _stored(ref, op, y):
    import srv_ref
    f32_out = srv_ref.gi(op, "o") == ref.out_tid or (op["kind"] == "deconv" and srv_ref.gi(op, "cout") == 1)
    return y.astype(np.float32).astype(np.float64) if f32_out else srv_ref.f16(y)


@pytest.mark.parametrize("net", sorted(SHAPES))
def test_checker_accepts_the_rounded_reference(built, net):
    import srv_ref
    ref, t = _f16_inputs(net, 4)
    for op in ref.ops:
        if op["kind"] == "output":
            continue
        y, bound = ref.op(op, t)
        assert srv_ref.ratio(_stored(ref, op, y), y, bound) <= 1.0, srv_ref.kind_of(op)


def test_checker_rejects_six_mutations(built):
    """each mutation, applied to the reference and rounded to f16 like a device result, fails the unmutated check.  The plans'
    average pools are unpadded (count_include_pad changes nothing there): that mutation is shown on a padded 3 x 3 window"""
    import srv_ref
    refs = {net: _f16_inputs(net, 5) for net in SHAPES}
    seen = {}
    for mut in srv_ref.MUTATIONS:
        for net, (ref, t) in refs.items():
            op = srv_ref.mutation_site(ref, mut)
            if op is None:
                continue
            y, bound = ref.op(op, t)
            ym, _ = ref.op(op, t, mut={mut: True})
            seen[mut] = srv_ref.ratio(_stored(ref, op, ym), y, bound)
            break
    assert srv_ref.mutation_site(refs["srv_det"][0], "avg_include_pad") is None
    ref, _ = refs["srv_det"]
    op = dict(kind="pool", kv=dict(kh="3", kw="3", sh="1", sw="1", ph="1", pw="1", type="avg"), ep=[])
    x = srv_ref.f16(np.random.RandomState(6).randn(1, 9, 11, 16))
    y, bound = ref.pool(op, x)
    ym, _ = ref.pool(op, x, mut={"avg_include_pad": True})
    seen["avg_include_pad"] = srv_ref.ratio(srv_ref.f16(ym), y, bound)
    print(" ".join("%s %.1f" % kv for kv in seen.items()))
    assert set(seen) == set(srv_ref.MUTATIONS), seen
    assert min(seen.values()) > 1.0, seen


def test_gelu_fit_of_the_f16_kernels():
    """srv_gelu8 (the f16 build's GELU): the fit restated in srv_ref.gelu_fit is within the 1.9e-4 its comment states of the exact GELU"""
    import torch
    import srv_ref
    x = np.linspace(-12, 12, 200001)
    exact = torch.nn.functional.gelu(torch.from_numpy(x)).numpy()
    assert np.abs(srv_ref.gelu_fit(x) - exact).max() <= srv_ref.GELU_FIT_ERR
