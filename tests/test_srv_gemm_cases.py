"""CPU half of the server GEMM family's own tests: the case table of tests/srv_gemm_cases.py really holds an op per designed branch
(recomputed from the shapes), the three references agree on every plan and shape, the predicted refusals give every configuration
its coverage, and every srv_ref.GEMM_MUTATIONS entry changes the reference by more than its bound somewhere on the table."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import srv_gemm_cases as G  # noqa: E402

ALL = [(name, shape) for name in "ABC" for shape in G.SHAPES[name]] + [("T%d" % c[1], s) for c in G.CTC_HEADS for s in G.CTC_SHAPES]
_RUNS = {}


def _oracle_run(name, shape):
    """(plan object, text, weights, x, oracle tensors tid -> f32 NHWC) - computed once per (plan, shape)"""
    import oracle as O
    key = (name, shape)
    if key not in _RUNS:
        P = G.plan(name, shape)
        text = P.text()
        Wt = P.weights(text)
        x = G.x_of(name, shape)
        net = O.OracleNet("synthetic", weights=Wt, plan=text)
        net.run(x)
        t = {op["o"]: net.tensor(op["o"]) for op in P.ops if op["live"]}
        _RUNS[key] = (P, text, Wt, x, t)
    return _RUNS[key]


def test_every_designed_branch_is_in_the_table():
    A = G.plan("A")
    ops = {op["label"]: op for op in A.ops}
    geo = lambda label, half=True, shape=(2, 8, 16): G.geometry(ops[label], shape, half)
    # linears: nkt, x1, column counts
    assert (geo("l64_64")["nkt"], geo("l64_64")["x1"]) == (1, 1)
    assert geo("l128_72")["ncols"] % 64 == 8 and geo("l128_72")["x1"] == 1
    assert geo("l192_200")["nkt"] == 3
    g = geo("l448_13")
    assert g["nkt"] == 7 and g["ncols"] % 8 == 5 and G.up8(13) - 13 == 3
    g = geo("l24_264")
    assert g["K"] == 24 and g["nkt"] == 1 and g["x1"] == 0 and g["cin_shift"] == -2
    assert geo("l96_576")["ncols"] % 192 == 0 and geo("l96_576")["ncols"] % 256 == 64 and geo("l96_576")["x1"] == 0
    # epilogues on the 128 -> 72 linear
    eps = {op["label"]: op["text"].split("ep=")[1] for op in A.ops if op["label"].startswith("e_") and op["role"] == "test"}
    kinds = {k: {s.split(":")[0] + (":" + s.split(":")[1] if s.startswith("act") else "") for s in v.split("|")} for k, v in eps.items()}
    assert kinds["e_bias"] == {"bias"} and kinds["e_bn"] == {"bn"} and kinds["e_bias_bn"] == {"bias", "bn"} and "addt" in kinds["e_addt"]
    assert {a for v in kinds.values() for a in v if a.startswith("act")} == {"act:" + a for a in G.ACTS}
    assert ops["out"]["role"] == "out" and ops["out"]["kind"] == "linear"
    # conv forms
    assert geo("c3_3")["cin_shift"] == 3 and geo("c3_24")["cin_shift"] == -2 and geo("c3_32")["cin_shift"] == 5
    assert geo("c3_32", half=False)["cin_shift"] == -1  # (the twin's K tile is 32 elements)
    for lb in ("c3_64", "c3_128"):
        assert (geo(lb)["cin_shift"], geo(lb)["korder"], geo(lb, half=False)["korder"]) == (-1, 1, 0)
        assert G.predicted_refusal(dict(form="halo"), ops[lb]) is None
    assert geo("c3_64_s2")["s"] == (2, 2) and geo("c3_64_s2")["korder"] == 1 and G.predicted_refusal(dict(form="halo"), ops["c3_64_s2"])
    assert (geo("c1_64_s2")["k"], geo("c1_64_s2")["s"], geo("c1_64_s2")["x1"]) == ((1, 1), (2, 2), 0)
    assert geo("c1x3_32")["k"] == (1, 3) and geo("c1x3_32")["p"] == (0, 1)
    assert geo("c3x1_32")["k"] == (3, 1) and geo("c3x1_32")["s"] == (2, 1) and geo("c3x1_32")["p"] == (1, 0)
    assert geo("c5_3")["k"] == (5, 5) and geo("c5_3")["nkt"] == 4
    assert geo("d64_64")["ncols"] == 256 and geo("d32_24")["ncols"] == 96 and G.parse_op(ops["d64_1"])[1]["cout"] == 1
    # every op under test with an f16 output has its follower
    for op in A.tests():
        if op["role"] == "test" and not op["label"] == "d64_1":
            assert any(f["of"] == op["label"] for f in A.ops if f["role"] == "follower"), op["label"]
    # the shapes: M around every BM, image borders inside a pixel tile with N > 1, a single-column map
    Ms = sorted(n * h * w for n, h, w in G.SHAPES["A"])
    assert Ms == [1, 63, 65, 255, 256, 257, 513]
    assert any(n > 1 and (h * w) % 64 for n, h, w in G.SHAPES["A"]) and any(w == 1 and h > 1 for _, h, w in G.SHAPES["A"])
    # plan B: addup, concat depths 1 - 4 (each at a shape with partial halo tiles and at N > 1), the head-tail pair
    depth_shapes = {d: [] for d in (1, 2, 3, 4)}
    for shape in G.SHAPES["B"]:
        B = G.plan("B", shape)
        live = {op["label"] for op in B.ops if op["live"]}
        assert {"u_lin", "u_relu", "u_c3", "ht1", "out"} <= live
        for d in depth_shapes:
            if "cat%d_c3" % d in live:
                depth_shapes[d].append(shape)
        b = {op["label"]: op for op in B.ops}
        assert "addup:" in b["u_lin"]["text"] and "addup:" in b["u_c3"]["text"] and G.predicted_refusal(dict(form="halo"), b["u_c3"])
        assert b["out"]["text"].startswith("i=%d " % b["ht1"]["o"]) and sum((" i=%d " % b["ht1"]["o"]) in (" " + o["text"]) for o in B.ops) == 1
    for d, shp in depth_shapes.items():
        assert any(h % 16 or w % 16 for _, h, w in shp) and any(n > 1 for n, _, _ in shp) and any(h > 16 or w > 16 for _, h, w in shp), (d, shp)
    assert [tuple(int(u) for u in G.parse_op(op)[0]["up"].split(",")) for op in G.plan("B", (1, 24, 40)).ops if op["kind"] == "concat"] == list(G.CAT_UPS)
    # plan C: the MLP pairs, token counts around the 128-token tile
    assert sorted(n * h * w for n, h, w in G.SHAPES["C"]) == [1, 127, 128, 129, 129] and (3, 1, 43) in G.SHAPES["C"]
    c = {op["label"]: G.parse_op(op)[1] for op in G.plan("C").ops}
    for C in G.MLP_WIDTHS:
        assert (c["fc1_%d" % C]["cin"], c["fc1_%d" % C]["cout"], c["fc2_%d" % C]["cout"]) == (C, 4 * C, C)
    assert [h[1] for h in G.CTC_HEADS] == [13, 64, 200]


def test_predicted_refusals_give_every_configuration_its_coverage(built, pkg):
    """conditions, not measurements: from the library's own table and the predicted refusals, every configuration that takes linears
    runs one with a partial last M tile and one with a partial last column tile (on the ring: nkt below, at and above its NS), every
    configuration that takes convs runs every conv form it accepts, and no op is refused by every configuration"""
    cfgs = pkg.SrvNet.configs()
    assert len(cfgs) >= 21 and all(bn % 64 == 0 for _, _, bn in cfgs)
    tiles = {cid: G.tile_of(name) for cid, name, _ in cfgs}
    assert {t["form"] for t in tiles.values()} == {"gemm", "reg", "halo"}
    for cid, name, bn in cfgs:
        assert tiles[cid]["BN"] == bn
    plans = [("A", s, G.plan("A")) for s in G.SHAPES["A"]] + [("B", s, G.plan("B", s)) for s in G.SHAPES["B"]]
    all_forms = {G.conv_form(op) for _, _, P in plans for op in G.gemm_ops(P) if op["kind"] == "conv" and op["role"] == "test"}
    assert len(all_forms) >= 9, all_forms
    never = {(pn, op["label"]) for pn, _, P in plans for op in G.gemm_ops(P)}
    for cid, t in tiles.items():
        part_m = part_n = False
        nkts, forms = set(), set()
        for pn, shape, P in plans:
            for op in G.gemm_ops(P):
                if G.predicted_refusal(t, op) is not None:
                    continue
                never.discard((pn, op["label"]))
                g = G.geometry(op, shape, True)
                if op["kind"] == "linear" and op["role"] == "test":
                    part_m |= g["M"] % t["BM"] != 0 and g["M"] > t["BM"]
                    part_n |= g["ncols"] % t["BN"] != 0 and g["ncols"] > t["BN"]
                    nkts.add(g["nkt"])
                if op["kind"] == "conv" and op["role"] == "test":
                    forms.add(G.conv_form(op))
        if t["form"] == "halo":
            assert forms == {"k3x3 s1x1 shift-1 order1"}, forms   # (takes no linear: its partial tiles are the 18 x 34 map's and the 72-column conv's)
            continue
        assert part_m and part_n, (cid, part_m, part_n)
        assert forms == all_forms, (cid, all_forms - forms)
        assert min(nkts) < t["NS"] < max(nkts), (cid, nkts)   # (the ring shrinks below NS and wraps above it)
    assert not never, never


@pytest.mark.parametrize("name,shape", ALL)
def test_three_references_agree(built, name, shape):
    """OracleNet(plan=...) against Ref(half=False) per op on the oracle's own inputs: bit for bit where Ref states the op exact, inside
    Ref's f32 bound elsewhere; torch_run (float64, from the grammar alone) within 2e-4 of every tensor's scale"""
    import srv_ref
    P, text, Wt, x, t = _oracle_run(name, shape)
    ref = srv_ref.Ref(text, Wt, half=False)
    t64 = {k: v.astype(np.float64) for k, v in t.items()}
    t64[0] = x.astype(np.float64)
    res = srv_ref.check_tensors(ref, t64)
    bad = {k: v for k, v in res.items() if not v[1] <= 1.0}
    assert not bad, bad
    out, tt = srv_ref.torch_run(text, Wt, x)
    for tid, w in tt.items():
        assert t[tid].shape == w.shape, (tid, t[tid].shape, w.shape)
        assert np.abs(t[tid] - w).max() <= 2e-4 * (np.abs(w).max() + 1e-9), tid


def test_every_gemm_mutation_separates_on_the_table(built):
    """each mutated reference differs from the oracle's result by more than the f32 bound on at least one (plan, shape) - so a
    device result that followed the mutation would be rejected"""
    import srv_ref
    worst = {m: 0.0 for m in srv_ref.GEMM_MUTATIONS}
    for name, shape in ALL:
        if name not in "AB":
            continue
        P, text, Wt, x, t = _oracle_run(name, shape)
        ref = srv_ref.Ref(text, Wt, half=False)
        t64 = {k: v.astype(np.float64) for k, v in t.items()}
        t64[0] = x.astype(np.float64)
        for mut in srv_ref.GEMM_MUTATIONS:
            for op in srv_ref.gemm_mutation_sites(ref, mut):
                worst[mut] = max(worst[mut], mutated_ratio(ref, op, t64, mut))
    print("GEMM mutations, worst err/bound over the table: " + "  ".join("%s %.3g" % kv for kv in worst.items()))
    assert min(worst.values()) > 1.0, worst


def mutated_ratio(ref, op, t, mut):
    """max |result - mutated reference| / bound of the op the mutation shows in (a concat's: the 3x3 conv that reads it)"""
    import srv_ref
    if op["kind"] == "concat":
        conv = next(o for o in ref.ops if o["kind"] == "conv" and srv_ref.gi(o, "i") == srv_ref.gi(op, "o"))
        tt = dict(t)
        tt[srv_ref.gi(op, "o")] = ref.op(op, t, mut={mut: True})[0]
        y, b = ref.op(conv, tt)
        return srv_ref.ratio(t[srv_ref.gi(conv, "o")], y, b)
    y, b = ref.op(op, t, mut={mut: True})
    return srv_ref.ratio(t[srv_ref.gi(op, "o")], y, b)
