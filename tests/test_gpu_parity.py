"""Parity tests proper: the HIP path through the C-ABI against the CPU oracle on the same seeded
inputs.  Bars: bit-exact for bytes / integers / indices (resized image, bitmap, boxes, CTC ids) AND for
the f32 maps, logits and scores — the kernels implement the oracle's arithmetic contract exactly
(DESIGN.md section 4), so `==` is the comparison, tighter than the 1e-3 the north star allows."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_native_library_is_loaded(pkg, built):
    import ctypes
    pkg.check(pkg.lib().ocr_rt_init(0))
    maps = open("/proc/self/maps").read()
    assert "libocr_hip.so" in maps  # the in-tree HIP library, not a fallback


def test_numerics_probe_matches_ieee_and_contract(pkg, built):
    import oracle as O
    rs = np.random.RandomState(0)
    a = np.concatenate([rs.randn(4096) * 10, rs.rand(4096) * 100 - 50, [0.0, -0.0, 1.0, 88.5, -90.0, 1e-30]]).astype(np.float32)
    b = (rs.randn(a.size) * 3 + 0.01).astype(np.float32)
    out = pkg.probe(a, b)
    assert np.array_equal(out[0], a / b)                      # correctly rounded division
    assert np.array_equal(out[1], np.sqrt(np.abs(a)))         # correctly rounded sqrt
    ref_exp = np.array([O.lib().oracle_expf(float(v)) for v in a], np.float32)
    assert np.array_equal(out[2], ref_exp)                    # the contract's exp, bit for bit
    assert np.array_equal(out[3], (a.astype(np.float64) * b + a).astype(np.float32))  # fma: one rounding
    assert np.array_equal(out[4], (a * b) + a)                # a*b+a is NOT contracted (-ffp-contract=off)


def _hswish_contract(y):
    """ocr_act(ACT_HSWISH): t = clamp(y + 3, 0, 6); u = y * t; u / 6, every step rounded to f32."""
    y = y.astype(np.float32)
    with np.errstate(all="ignore"):
        t = np.minimum(np.maximum(y + np.float32(3), np.float32(0)), np.float32(6))
        return (y * t) / np.float32(6)


def test_hswish_division_free_path_is_the_division(pkg, built):
    """The epilogues replace u/6 by q0 = u*r, e = fma(-6, q0, u), q = fma(e, r, q0) behind a range guard
    (ocr_common.h; tools/check_div6.c is the exhaustive CPU proof of the identity).  Here: the device code
    itself on ordinary values and on every kind of edge - zeros of both signs, denormals, the binades where
    the quotient goes denormal, exact ties among denormal quotients, huge values whose u overflows,
    infinities - bit for bit against the contract's division."""
    rs = np.random.RandomState(1)
    bits = lambda v: np.asarray(v, np.float32).view(np.uint32)
    edge = np.array([0.0, -0.0, 3e-45, -3e-45, 1e-39, -1e-39, 1.1754944e-38, -1.1754944e-38, 2e-38, 1e-37, -1e-36,
                     1e-30, 5e37, 5.7e37, -5.7e37, 1e38, -1e38, 3.4e38, np.inf, -np.inf, -3.0, -3.0000002, -2.9999998,
                     3.0, 2.9999998, 3.0000002, 6.0, -6.0], np.float32)
    ties = (np.arange(1, 4000, dtype=np.uint32) * 2 + 1).view(np.float32)          # odd multiples of 2^-149
    tiny = (rs.randint(1, 0x02000000, 20000).astype(np.uint32) | (rs.randint(0, 2, 20000).astype(np.uint32) << 31)).view(np.float32)
    a = np.concatenate([edge, ties, -ties, tiny, rs.randn(60000).astype(np.float32) * 4,
                        (rs.rand(20000).astype(np.float32) - 0.5) * 1e-3]).astype(np.float32)
    b = np.concatenate([rs.randn(a.size - 3000).astype(np.float32) * 3, tiny[:3000]]).astype(np.float32)
    out = pkg.probe(a, b)
    want_a, want_b = _hswish_contract(a), _hswish_contract(b)
    same = lambda g, w: (bits(g) == bits(w)) | (np.isnan(g) & np.isnan(w))
    assert same(out[6], want_a).all(), a[~same(out[6], want_a)][:8]
    assert same(out[7], want_b).all(), b[~same(out[7], want_b)][:8]


@pytest.mark.parametrize("kind,shape", [("cls", (5, 48, 192)), ("det", (3, 96, 128)), ("rec", (5, 48, 320)), ("rec", (2, 28, 192))])
def test_production_mode_output_bit_identical(pkg, built, kind, shape):
    """keep_all=False is what the stages run: liveness-reused arena, and the SE gate multiplies folded into
    the 1x1 convs that read them (net.hip, `folded`).  Several images per launch so that the per-image gate
    rows matter; the final output must still equal the oracle's bit for bit."""
    from oracle import OracleNet
    x = np.random.RandomState(11).randn(shape[0], shape[1], shape[2], 3).astype(np.float32)
    o = OracleNet(kind)
    g = pkg.Net(kind)
    yo, yg = o.run(x), g.forward(x, keep_all=False)
    assert yo.shape == yg.shape and np.array_equal(yo, yg)
    g.close()


_AB_CHILD = r"""
import sys, numpy as np
sys.path[:0] = [sys.argv[1], sys.argv[1] + "/oracle", sys.argv[1] + "/tools"]
import __graft_entry__ as ge
pkg = ge.load_package()
from oracle import OracleNet
for kind, shape in (("det", (2, 96, 160)), ("det", (1, 192, 384)), ("rec", (3, 48, 320)), ("rec", (5, 48, 136)), ("rec", (2, 28, 192)),
                    ("cls", (2, 48, 192))):
    x = np.random.RandomState(3).randn(shape[0], shape[1], shape[2], 3).astype(np.float32)
    o, g = OracleNet(kind), pkg.Net(kind)
    assert np.array_equal(o.run(x), g.forward(x, keep_all=False)), (kind, shape)
    g.close()
# the recognizer's production path: a ragged batch (own width per line) against each line alone
rs = np.random.RandomState(4)
lines = [rs.randn(48, w, 3).astype(np.float32) for w in (320, 320, 333, 136, 320, 350)]
o, g = OracleNet("rec"), pkg.Net("rec")
want = np.concatenate([o.run(l[None]).reshape(-1, 6625) for l in lines])
assert np.array_equal(want, g.forward_ragged(lines, keep_all=False).reshape(-1, 6625)), "ragged rec"
g.close()
# the detector's path for mixed sizes: a ragged batch of images against each image alone (needs the fused DB head)
import os
if os.environ.get("OCR_FUSE") != "0":
    imgs = [rs.randn(h, w, 3).astype(np.float32) for h, w in ((96, 160), (64, 64), (32, 96), (160, 96), (64, 64), (128, 224))]
    o, g = OracleNet("det"), pkg.Net("det")
    want = np.concatenate([o.run(im[None]).reshape(-1) for im in imgs])
    assert np.array_equal(want, g.forward_ragged_images(imgs, keep_all=False).reshape(-1)), "ragged det"
    g.close()
print("AB OK")
"""


# every switch of csrc/rt_options.h (INTEGRATION.md's table), each in the setting that is NOT the default
_AB_ENVS = [{"OCR_FUSE": "0"}, {"OCR_FUSE_GAP_MIN": "1", "OCR_CONV_MT2": "force"}, {"OCR_CONV_SMALL_NT": "0", "OCR_CONV_MT2": "0", "OCR_CONV_C24": "0"},
            {"OCR_DW_LDS": "0", "OCR_ATTN_LINE": "0"}, {"OCR_XDW": "0"}, {"OCR_DWPW2": "0"}, {"OCR_DWPW2": "0", "OCR_DWPW_FORCE_UPW": "3"},
            {"OCR_DWPW_T4": "thin"}, {"OCR_DWPW_ITEMS": "7"}, {"OCR_DWPW_ITEMS": "1"}, {"OCR_DWPW_FORCE_UPW": "3"},
            {"OCR_DWPW_FORCE_UPW": "16", "OCR_DWPW_T4": "thin"},
            # not a switch but another BUILD (build.py --variant vmcnt0): every hand-counted s_waitcnt vmcnt(N) of the LDS-DMA fused-block
            # kernel as vmcnt(0).  Both builds equal the oracle, hence each other: the counts are not too large on these shapes
            {"OCR_LIB_PATH": os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cpp-paddle-ocr_amd", "lib", "libocr_hip_vmcnt0.so")},
            {"OCR_LIB_PATH": os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cpp-paddle-ocr_amd", "lib", "libocr_hip_vmcnt0.so"),
             "OCR_DWPW_ITEMS": "7", "OCR_DWPW_FORCE_UPW": "3"}]


_AB_RESULTS = {}


def _ab_run_all():
    """the twelve child processes are independent: four at a time (the box allows six processes on the card, this one included) -
    the suite's wall time was 468 s of a 900 s limit with them one after the other"""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pending = list(enumerate(_AB_ENVS))
    running = []
    while pending or running:
        while pending and len(running) < 4:
            i, env = pending.pop(0)
            running.append((i, subprocess.Popen([sys.executable, "-c", _AB_CHILD, root], env=dict(os.environ, **env), stdout=subprocess.PIPE,
                                                stderr=subprocess.PIPE, text=True)))
        i, pr = running.pop(0)
        try:
            so, se = pr.communicate(timeout=900)
        except subprocess.TimeoutExpired:
            pr.kill()
            so, se = pr.communicate()
            se += "\nTIMEOUT"
        _AB_RESULTS[i] = (pr.returncode, so, se)


@pytest.mark.parametrize("idx", range(len(_AB_ENVS)), ids=["-".join("%s=%s" % (k, os.path.basename(v)) for k, v in e.items()) for e in _AB_ENVS])
def test_ab_switches_do_not_change_results(built, idx):
    """INTEGRATION.md's runtime switches select other kernel shapes / launch lists (read once per process, so each
    setting runs in a child process): the production-mode outputs stay bit-identical to the oracle.  OCR_DWPW_ITEMS = 7
    and 1 give workgroups odd and single-item pipelines (the peeled first / last iterations of kernels_dwpw.hip);
    OCR_DWPW_FORCE_UPW gives the workgroups of these small inputs several units each (production batches have 2-32:
    unit boundaries inside a pipeline, a shorter last workgroup); OCR_FUSE_GAP_MIN = 1 sends these small batches down the depthwise-conv-with-row-sums path that otherwise starts at
    64 k bands (production batches).  The children of all settings run four at a time; every test reads its own child's verdict."""
    if not _AB_RESULTS:
        _ab_run_all()
    rc, so, se = _AB_RESULTS[idx]
    assert rc == 0 and "AB OK" in so, so[-2000:] + se[-2000:]


_LAUNCH_LISTS = {}


@pytest.mark.parametrize("group", ["cases", "gap_min1_mt2_force", "fuse0"])
def test_binder_decisions_equal_the_recorded_launch_lists(built, group):
    """What Net::bind decides is invisible to the bit-exact tests above (a launch moved to another launcher gives the same
    numbers): tools/net_launch_list.py lists, per case, every launch of one forward (name, count, flops, bytes) and which plan
    tensors exist.  tests/golden/net_launch_lists.json is its output at the commit before bind was split into phases; the same
    tool now must give exactly that - uniform fp32 / fp16 batches at keep_all 0, 1, 2, both ragged forms, one Pipe run, and
    the det / rec cases again under two switch sets (one child process each, started together with the main cases)."""
    import json
    import net_launch_list
    if not _LAUNCH_LISTS:
        _LAUNCH_LISTS.update(net_launch_list.collect_all())
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "net_launch_lists.json")))
    want, got = (want["cases"], _LAUNCH_LISTS["cases"]) if group == "cases" else (want["switches"][group], _LAUNCH_LISTS["switches"][group])
    assert sorted(got) == sorted(want)
    for key in sorted(want):
        assert got[key] == want[key], key


@pytest.mark.parametrize("kind,shape", [("det", (2, 96, 160)), ("det", (1, 192, 384)), ("det", (3, 64, 64)), ("rec", (3, 48, 320)),
                                        ("rec", (2, 28, 192)), ("rec", (1, 48, 1000)), ("rec", (5, 48, 136)), ("cls", (3, 48, 192))])
def test_fused_launch_list_every_materialised_tensor_bit_identical(pkg, built, kind, shape):
    """keep_all=2 runs the PRODUCTION launch list (SE gates folded into 1x1 convs, depthwise -> pointwise pairs fused
    into one launch: kernels_dwpw.hip) but gives every tensor its own slot: each tensor the fused list still writes
    must equal the oracle's, and the fused-away ones must be exactly the depthwise outputs / gated products.
    Shapes include maps that are not multiples of the 8x16 / 4x16 tiles and single-row-pair maps."""
    from oracle import OracleNet
    x = np.random.RandomState(5).randn(shape[0], shape[1], shape[2], 3).astype(np.float32)
    o = OracleNet(kind)
    g = pkg.Net(kind)
    yo, yg = o.run(x), g.forward(x, keep_all=2)
    assert yo.shape == yg.shape and np.array_equal(yo, yg)
    missing = 0
    for tid in range(1, g.num_tensors()):
        to = o.tensor(tid)
        if not to.size:
            continue
        if g.exists(tid):
            assert np.array_equal(to, g.fetch(tid)), "tensor %d" % tid
        else:
            missing += 1
    if kind in ("det", "rec"):
        assert missing >= 8          # the fused pairs really ran fused
    g.close()


@pytest.mark.parametrize("keep_all", [0, 1, 2])
@pytest.mark.parametrize("h,widths", [(48, [320, 320, 327, 345, 40, 320, 1000, 64, 321]), (28, [192, 201, 192, 77])])
def test_ragged_rec_batch_equals_each_line_alone(pkg, built, keep_all, h, widths):
    """The recognizer runs ONE launch list per call: every line keeps its own tensor width (the width of its batch of
    rec_batch_num, src/ocr_rec.cpp:47-72) inside a ragged batch (kernels_net.h, RagLevel).  Every tensor of every
    line must equal what the oracle computes for that line alone - in all three launch-list modes (production,
    every plan tensor materialised, production list with every written tensor kept).  Widths include odd ones
    (odd widths at every level), a very wide line, lines narrower than a 16-pixel tile row and equal neighbours."""
    from oracle import OracleNet
    rs = np.random.RandomState(31)
    lines = [rs.randn(h, w, 3).astype(np.float32) for w in widths]
    o = OracleNet("rec")
    g = pkg.Net("rec")
    y = g.forward_ragged(lines, keep_all=keep_all)
    nt = g.num_tensors()
    outs, taps = [], {t: [] for t in range(1, nt)}
    for l in lines:
        outs.append(o.run(l[None]))
        if keep_all:
            for t in range(1, nt):
                taps[t].append(o.tensor(t).copy())
    C = outs[0].shape[-1]
    assert np.array_equal(np.concatenate([v.reshape(-1, C) for v in outs]), y.reshape(-1, C))
    checked = 0
    for t in range(1, nt if keep_all else 1):
        if not taps[t][0].size or not g.exists(t):
            continue
        c = taps[t][0].shape[-1]
        assert np.array_equal(np.concatenate([v.reshape(-1, c) for v in taps[t]]), g.fetch(t).reshape(-1, c)), "tensor %d" % t
        checked += 1
    assert checked >= (40 if keep_all else 0)
    # the same binding again with new contents, then another composition, then the first one (cached binding + tables)
    lines2 = [rs.randn(h, w, 3).astype(np.float32) for w in widths]
    want2 = np.concatenate([o.run(l[None]).reshape(-1, C) for l in lines2[:3]])
    assert np.array_equal(want2, g.forward_ragged(lines2[:3], keep_all=keep_all).reshape(-1, C))
    assert np.array_equal(np.concatenate([v.reshape(-1, C) for v in outs]), g.forward_ragged(lines, keep_all=keep_all).reshape(-1, C))
    g.close()


@pytest.mark.parametrize("keep_all", [0, 2])
def test_ragged_det_batch_equals_each_image_alone(pkg, built, keep_all):
    """The detector on a batch of MIXED sizes runs one launch list for all of them (kernels_net.h, RagLevel with heights;
    Net::run_ragged_images): every image keeps its own height and width - zero padding, SE pools, FPN upsampling, the
    8x16 LDS tiles and the DB head's 4x4 expansion all take the image's own size.  Every tensor the production list
    writes, and the probability map, must equal what the oracle computes for that image alone.  Sizes include the
    smallest (32), non-square, equal neighbours and sizes that are not multiples of the tile shapes at the coarse levels."""
    from oracle import OracleNet
    rs = np.random.RandomState(41)
    sizes = [(96, 160), (96, 160), (32, 32), (64, 224), (160, 96), (128, 128), (32, 96), (224, 64)]
    imgs = [rs.randn(h, w, 3).astype(np.float32) for h, w in sizes]
    o = OracleNet("det")
    g = pkg.Net("det")
    y = g.forward_ragged_images(imgs, keep_all=keep_all)
    nt = g.num_tensors()
    outs, taps = [], {t: [] for t in range(1, nt)}
    for im in imgs:
        outs.append(o.run(im[None]))
        if keep_all:
            for t in range(1, nt):
                taps[t].append(o.tensor(t).copy())
    assert np.array_equal(np.concatenate([v.reshape(-1) for v in outs]), y.reshape(-1))
    checked = 0
    for t in range(1, nt if keep_all else 1):
        if not taps[t][0].size or not g.exists(t):
            continue
        c = taps[t][0].shape[-1]
        assert np.array_equal(np.concatenate([v.reshape(-1, c) for v in taps[t]]), g.fetch(t).reshape(-1, c)), "tensor %d" % t
        checked += 1
    assert checked >= (40 if keep_all else 0)
    # another composition, then the first again (cached binding and tables), then a uniform batch on the same handle
    sub = [imgs[i] for i in (4, 0, 7)]
    want = np.concatenate([o.run(im[None]).reshape(-1) for im in sub])
    assert np.array_equal(want, g.forward_ragged_images(sub, keep_all=keep_all).reshape(-1))
    assert np.array_equal(np.concatenate([v.reshape(-1) for v in outs]), g.forward_ragged_images(imgs, keep_all=keep_all).reshape(-1))
    x = np.stack([imgs[0], imgs[1]])
    assert np.array_equal(o.run(x), g.forward(x, keep_all=keep_all))
    g.close()


@pytest.mark.parametrize("graph", ["1", "0"])
@pytest.mark.parametrize("kind,shape,other", [("rec", (3, 48, 160), (2, 48, 96)), ("det", (2, 64, 96), (1, 96, 64)),
                                              ("cls", (4, 48, 192), (1, 48, 192))])
def test_repeated_runs_of_a_binding_track_their_input(pkg, built, monkeypatch, graph, kind, shape, other):
    """A binding is run plainly once, recorded into a hipGraph when the same input buffer comes back, and replayed
    afterwards (Net::run).  Six runs of one shape with NEW contents each time, a different shape in between (the
    cached binding and its graph must survive the switch), every run compared with the oracle; the same with
    graphs off."""
    from oracle import OracleNet
    monkeypatch.setenv("OCR_GRAPH", graph)
    o = OracleNet(kind)
    g = pkg.Net(kind)
    rs = np.random.RandomState(23)
    for it in range(6):
        x = rs.randn(shape[0], shape[1], shape[2], 3).astype(np.float32)
        assert np.array_equal(o.run(x), g.forward(x, keep_all=False)), "run %d" % it
        if it in (2, 4):
            y = rs.randn(other[0], other[1], other[2], 3).astype(np.float32)
            assert np.array_equal(o.run(y), g.forward(y, keep_all=False)), "other shape after run %d" % it
    g.close()


def test_refused_launch_is_an_error_code_not_an_abort(pkg, built, card):
    """A launcher that refuses a shape the binding had accepted (cannot happen by construction; rounds 1-2 called abort())
    fails the run with OCR_ERR_DEVICE and a message - through the raw network tap and through the pipeline - and the
    handle keeps working afterwards.  Driven by the library's fault-injection hook."""
    L = pkg.lib()
    x = np.random.RandomState(1).randn(2, 48, 192, 3).astype(np.float32)
    g = pkg.Net("rec")
    want = g.forward(x, keep_all=False)
    pg = pkg.Pipe()
    ok_words = pg.run([card, card])
    try:
        assert L.ocr_selftest_refuse_launch(b"dwpw3x3_64_64") == 0
        with pytest.raises(pkg.OcrError, match=r"error -3: .*refused"):
            g.forward(x, keep_all=False)
        with pytest.raises(pkg.OcrError, match=r"error -3: .*refused"):
            pg.run([card, card])
    finally:
        L.ocr_selftest_refuse_launch(None)
    assert np.array_equal(want, g.forward(x, keep_all=False))
    again = pg.run([card, card])
    assert [len(w) for w in again] == [len(w) for w in ok_words]
    assert all(np.array_equal(a["ids"], b["ids"]) for wa, wb in zip(again, ok_words) for a, b in zip(wa, wb))
    g.close()
    pg.close()


def test_model_directory_with_another_graph_is_refused(pkg, built):
    """The compiled-in plan binds weights to layers by name: a model directory whose graph is not the one the plan was
    generated from (op count / op-type signature, pd_format.cpp) must fail at load, not run with misbound weights."""
    import os
    for kind, other in (("det", "cls"), ("cls", "rec"), ("rec", "det")):
        with pytest.raises(pkg.OcrError, match="is not the %s graph" % kind):
            pkg.Net(kind, model_dir=os.path.join(pkg.MODELS, other))
    with pytest.raises(pkg.OcrError, match="is not the det graph"):
        pkg.Det(model_dir=os.path.join(pkg.MODELS, "rec"))


@pytest.mark.parametrize("kind,shape", [("cls", (3, 48, 192)), ("det", (2, 64, 96)), ("det", (1, 192, 384)),
                                        ("rec", (3, 48, 160)), ("rec", (2, 28, 192)), ("rec", (1, 48, 1000))])
def test_network_outputs_bit_identical(pkg, built, kind, shape):
    from oracle import OracleNet
    x = np.random.RandomState(7).randn(shape[0], shape[1], shape[2], 3).astype(np.float32)
    o = OracleNet(kind)
    g = pkg.Net(kind)
    yo, yg = o.run(x), g.forward(x, keep_all=True)
    assert yo.shape == yg.shape and np.array_equal(yo, yg)
    # layer by layer (every plan tensor, converted back from the device's interleaved channel layout)
    for tid in range(1, g.num_tensors()):
        to = o.tensor(tid)
        if to.size:
            assert np.array_equal(to, g.fetch(tid)), "tensor %d" % tid
    g.close()


def test_det_on_reference_image_worker_defaults(pkg, built, card):
    """cfg1: card-jd.jpg, limit 512 / 0.2 / 0.4 / 1.8 / fast (ocr_worker.cpp:21-35)."""
    from pipeline import Pipeline
    pipe, det = Pipeline(), pkg.Det()
    bo, bg = pipe.det_run(card), det.run(card)
    assert det.last_shape() == (1, 192, 384)                  # 178x391 -> 192x384 (SURVEY 8 "cfg1")
    assert np.array_equal(det.resized(), pipe.taps["det_resized"])
    assert np.array_equal(det.prob_map(), pipe.taps["det_prob"])
    assert np.array_equal(det.bitmap(), pipe.taps["det_bitmap"])
    assert len(bo) == len(bg) > 0 and all(np.array_equal(a, b) for a, b in zip(bo, bg))
    # strided ROI view input (a cv::Mat ROI): same result as its contiguous copy
    big = np.zeros((200, 420, 3), np.uint8)
    big[10:188, 20:411] = card
    bv = det.run(big[10:188, 20:411])
    assert len(bv) == len(bg) and all(np.array_equal(a, b) for a, b in zip(bv, bg))
    det.close()


@pytest.mark.parametrize("dilate", [False, True])
def test_det_post_on_probability_maps(pkg, built, dilate):
    import oracle as O
    from scipy import ndimage
    from synth_data import cfg2_sample
    det = pkg.Det(limit_side_len=960, thresh=0.3, box_thresh=0.5, unclip_ratio=2.0, use_dilation=dilate)
    for i in range(3):
        _, prob, _ = cfg2_sample(i)
        bo, bg = O.det_post(prob, 0.3, 0.5, 2.0, 960, 960, dilate), det.post(prob, 960, 960)
        assert len(bo) == len(bg) == 32 and all(np.array_equal(a, b) for a, b in zip(bo, bg))
    rs = np.random.RandomState(3)
    for i in range(6):   # blobs, specks, holes, borders touching the frame; different source scale
        H, W = 224 + 32 * i, 320
        f = ndimage.gaussian_filter(rs.rand(H, W), 1.0 + i)
        f = ((f - f.min()) / (f.max() - f.min())) ** (1.5 + 0.5 * i)
        f = f.astype(np.float32)
        bo, bg = O.det_post(f, 0.3, 0.5, 2.0, 2 * H, 3 * W, dilate), det.post(f, 2 * H, 3 * W)
        assert len(bo) == len(bg) and all(np.array_equal(a, b) for a, b in zip(bo, bg))
    # edge cases: empty map, full map, single pixel, 1-px lines
    for f in (np.zeros((64, 96), np.float32), np.ones((64, 96), np.float32)):
        assert len(det.post(f, 64, 96)) == len(O.det_post(f, 0.3, 0.5, 2.0, 64, 96, dilate))
    f = np.zeros((64, 96), np.float32)
    f[10, 10] = 1
    f[20, 5:60] = 1
    f[30:50, 70] = 1
    f[40:60, 10:50] = 0.95
    bo, bg = O.det_post(f, 0.3, 0.5, 2.0, 64, 96, dilate), det.post(f, 64, 96)
    assert len(bo) == len(bg) and all(np.array_equal(a, b) for a, b in zip(bo, bg))
    det.close()


@pytest.mark.parametrize("dilate", [False, True])
def test_det_post_slow_score_mode(pkg, built, dilate):
    """det_db_score_mode="slow": PolygonScoreAcc over the contour itself (postprocess_op.cpp:170-214)."""
    import oracle as O
    from scipy import ndimage
    from synth_data import cfg2_sample
    det = pkg.Det(limit_side_len=960, thresh=0.3, box_thresh=0.6, unclip_ratio=2.0, use_dilation=dilate, score_mode="slow")
    for i in range(2):
        _, prob, _ = cfg2_sample(i)
        bo, bg = O.det_post(prob, 0.3, 0.6, 2.0, 960, 960, dilate, slow=True), det.post(prob, 960, 960)
        assert len(bo) == len(bg) > 0 and all(np.array_equal(a, b) for a, b in zip(bo, bg))
    rs = np.random.RandomState(11)
    for i in range(8):   # ragged blobs with holes and frame contact: polygon mask != box mask
        H, W = 192 + 64 * i, 352 + 32 * (i % 3)
        f = ndimage.gaussian_filter(rs.rand(H, W), 1.0 + 0.7 * i)
        f = (((f - f.min()) / (f.max() - f.min())) ** (1.2 + 0.3 * i)).astype(np.float32)
        bo, bg = O.det_post(f, 0.3, 0.6, 2.0, 2 * H, 3 * W, dilate, slow=True), det.post(f, 2 * H, 3 * W)
        assert len(bo) == len(bg) and all(np.array_equal(a, b) for a, b in zip(bo, bg))
    # ~900 ragged borders, the largest with 8-16 thousand vertices (> 4096: the global-memory sort path restores contour order)
    H = W = 960
    f = (ndimage.gaussian_filter(np.random.RandomState(5).rand(H, W), 3.0) > 0.5).astype(np.float32)
    f[0, :] = f[-1, :] = f[:, 0] = f[:, -1] = 1
    det2 = pkg.Det(limit_side_len=960, thresh=0.3, box_thresh=0.1, unclip_ratio=2.0, use_dilation=dilate, score_mode="slow")
    fast = pkg.Det(limit_side_len=960, thresh=0.3, box_thresh=0.1, unclip_ratio=2.0, use_dilation=dilate)
    bo, bg = O.det_post(f, 0.3, 0.1, 2.0, H, W, dilate, slow=True), det2.post(f, H, W)
    assert len(bo) == len(bg) > 500 and all(np.array_equal(a, b) for a, b in zip(bo, bg))
    if dilate:    # the mode is really a different score, not an alias of "fast"
        assert len(bg) != len(fast.post(f, H, W))
    det2.close()
    for z in (np.zeros((64, 96), np.float32), np.ones((64, 96), np.float32)):
        assert len(det.post(z, 64, 96)) == len(O.det_post(z, 0.3, 0.6, 2.0, 64, 96, dilate, slow=True))
    det.close()
    fast.close()


def test_det_post_border_walk_with_tiny_provisional_slices(pkg, built, monkeypatch):
    """The border walk stores vertices into a provisional slice while it counts them and walks a border again when
    the slice was too small (trace_lds_kernel): with 4-vertex slices every real border takes that path."""
    import oracle as O
    from synth_data import cfg2_sample
    _, prob, _ = cfg2_sample(4)
    det = pkg.Det(limit_side_len=960, thresh=0.3, box_thresh=0.5, unclip_ratio=2.0)
    want = O.det_post(prob, 0.3, 0.5, 2.0, 960, 960)
    for limit in ("4", "64", ""):
        monkeypatch.setenv("OCR_TRACE_SLICE", limit)
        got = det.post(prob, 960, 960)
        assert len(want) == len(got) == 32 and all(np.array_equal(a, b) for a, b in zip(want, got))
    det.close()


def test_det_post_large_working_set_fallback(pkg, built):
    """A border whose unclip polygon outgrows the small per-border LDS working set (256 points) is redone
    with the large one: same boxes as the oracle, no error."""
    import oracle as O
    f = np.zeros((960, 960), np.float32)
    f[60:900, 80:880] = 0.9                      # one huge box: delta = area * ratio / perimeter ~ 4100 px
    f[20:40, 20:300] = 0.9                       # and an ordinary one
    det = pkg.Det(limit_side_len=960, thresh=0.3, box_thresh=0.5, unclip_ratio=20.0)
    bo, bg = O.det_post(f, 0.3, 0.5, 20.0, 960, 960), det.post(f, 960, 960)
    assert len(bo) == len(bg) == 2 and all(np.array_equal(a, b) for a, b in zip(bo, bg))
    det.close()


def test_det_batch_full_size_and_determinism(pkg, built):
    """cfg2 size (960x960) with the full network on synthetic weights: batch == singles == oracle."""
    from pipeline import Pipeline, DetCfg
    from synth_data import cfg2_sample
    imgs = [cfg2_sample(i)[0] for i in range(3)]
    det = pkg.Det(limit_side_len=960, thresh=0.3, box_thresh=0.5, unclip_ratio=2.0, max_batch=3)
    batch = det.run_batch(imgs)
    prob1 = det.prob_map(1)
    again = det.run_batch(imgs)
    assert all(np.array_equal(a, b) for x, y in zip(batch, again) for a, b in zip(x, y))  # idempotent
    single = det.run(imgs[1])
    assert np.array_equal(det.prob_map(0), prob1)                                         # batch-invariant
    assert len(single) == len(batch[1]) and all(np.array_equal(a, b) for a, b in zip(single, batch[1]))
    po = Pipeline(det_cfg=DetCfg(limit_side_len=960, thresh=0.3, box_thresh=0.5, unclip_ratio=2.0))
    bo = po.det_run(imgs[1])
    assert np.array_equal(po.taps["det_prob"], prob1)
    assert len(bo) == len(single) and all(np.array_equal(a, b) for a, b in zip(bo, single))
    for b in batch:  # size-independent properties of FilterTagDetRes
        for q in b:
            assert (q >= 0).all() and (q[:, 0] <= 959).all() and (q[:, 1] <= 959).all()
            assert int(np.hypot(*(q[0] - q[1]))) > 4 and int(np.hypot(*(q[0] - q[3]))) > 4
    det.close()


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
            crops.append(img[y:y + h, x:x + w])   # ROI views with the parent's row stride
    return crops


@pytest.mark.parametrize("h,w,bn", [(48, 320, 6), (28, 192, 16)])
def test_rec_ids_scores_and_steps(pkg, built, h, w, bn):
    from pipeline import Pipeline
    crops = _crops()
    assert len(crops) == 32
    po = Pipeline(rec_batch_num=bn, rec_img_h=h, rec_img_w=w)
    rec = pkg.Rec(rec_batch_num=bn, rec_img_h=h, rec_img_w=w)
    to, so, steps = po.rec_run(crops)
    tg, sg = rec.run(crops)
    assert rec.num_classes() == 6625 and rec.label(0) == "#" and rec.label(6624) == " "
    assert all(np.array_equal(a, b) for a, b in zip(to, tg))     # CTC class ids: bit-exact
    assert np.array_equal(so, sg)                                # mean max-probability: bit-exact
    for i in range(len(crops)):
        am, pm = rec.steps(i)
        assert np.array_equal(am, steps[i][0]) and np.array_equal(pm, steps[i][1])
    # ragged / empty inputs
    assert rec.run([])[0] == []
    one = rec.run([crops[3]])
    assert len(one[0]) == 1
    rec.close()


def test_rec_cls_extreme_crops(pkg, built):
    """Single pixels, one-pixel-high strips, needle-thin columns, a crop exactly 2x the target size (the
    INTER_AREA switch of cv::resize) and very wide lines (tensor width above rec_img_w)."""
    from pipeline import Pipeline
    rs = np.random.RandomState(8)
    shapes = [(1, 1), (1, 300), (300, 1), (2, 2), (96, 640), (96, 384), (48, 320), (7, 1000), (13, 37), (200, 9)]
    crops = [rs.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in shapes]
    po = Pipeline(rec_batch_num=4, rec_img_h=48, rec_img_w=320, enable_cls=True)
    rec, cls = pkg.Rec(rec_batch_num=4, rec_img_h=48, rec_img_w=320), pkg.Cls()
    to, so, steps = po.rec_run(crops)
    tg, sg = rec.run(crops)
    assert all(np.array_equal(a, b) for a, b in zip(to, tg)) and np.array_equal(so, sg)
    for i in range(len(crops)):
        am, pm = rec.steps(i)
        assert np.array_equal(am, steps[i][0]) and np.array_equal(pm, steps[i][1])
    lo, sco = po.cls_run(crops)
    lg, scg = cls.run(crops)
    assert np.array_equal(lo, lg) and np.array_equal(sco, scg)
    rec.close()
    cls.close()


def test_cls_on_real_weights(pkg, built):
    from pipeline import Pipeline
    crops = _crops()
    po, cls = Pipeline(enable_cls=True), pkg.Cls()
    lo, so = po.cls_run(crops)
    lg, sg = cls.run(crops)
    assert np.array_equal(lo, lg) and np.array_equal(so, sg)
    assert np.array_equal(cls.probs(len(crops)), po.taps["cls_probs"])
    assert 0 < lg.sum() < len(crops)      # both orientations occur, so the rotate path is exercised below
    cls.close()


_ORACLE_CACHE = {}


@pytest.mark.parametrize("phases", [1, 2])
@pytest.mark.parametrize("cls_on", [False, True])
def test_pipeline_process_request(pkg, built, card, cls_on, phases):
    """OCRWorker::processRequest: ids kept per request, mixed sizes in one call, cls rotation in place.  phases = 2 (the
    default) runs the batch as two chains on two parts of it, each with its own stage objects and host thread
    (pipe.hip, ocr_pipe::run_images); phases = 1 as one chain: the results are the same."""
    from pipeline import Pipeline
    pg = pkg.Pipe(enable_cls=cls_on, phases=phases)
    imgs = [card, card[:, ::-1].copy(), card[:120].copy(), card]
    got = pg.run(imgs)
    # the oracle's answers do not depend on `phases`: computed once per cls setting (the CPU oracle is most of this suite's
    # wall time - 442 s of the driver's 900 s limit in round 6 - and these four parametrisations asked it the same questions)
    key = ("process_request", cls_on)
    if key not in _ORACLE_CACHE:
        po = Pipeline(enable_cls=cls_on)
        blank0 = np.full((64, 64, 3), 255, np.uint8)
        _ORACLE_CACHE[key] = ([po.process(img)["words"] for img in imgs[:3]], len(po.process(blank0)["words"]))
    want3, want_blank = _ORACLE_CACHE[key]
    for img, g, w in zip(imgs, got, want3 + [want3[0]]):
        assert len(g) == len(w)
        for a, b in zip(g, w):
            assert np.array_equal(a["box"], b["box"]) and np.array_equal(a["ids"], b["ids"])
            assert a["confidence"] == np.float32(b["confidence"])
    # an image without text: success with zero words (ocr_worker.cpp:235-241)
    blank = np.full((64, 64, 3), 255, np.uint8)
    assert len(pg.run([blank])[0]) == want_blank
    with pytest.raises(pkg.OcrError, match="Empty image"):
        pg.run([np.zeros((0, 0, 3), np.uint8)])
    pg.close()


def _random_quads(rs, rows, cols, n):
    """Rotated / sheared / tall text boxes inside a rows x cols image (x0,y0..x3,y3, clockwise from TL)."""
    out = []
    while len(out) < n:
        cx, cy = rs.uniform(0, cols), rs.uniform(0, rows)
        w, h = rs.uniform(3, cols / 2), rs.uniform(3, rows / 3)
        if rs.rand() < 0.25:
            w, h = h, w * 1.6                                      # tall: the 90-degree branch
        a = np.deg2rad(rs.uniform(-40, 40))
        ca, sa = np.cos(a), np.sin(a)
        q = np.array([[-w / 2, -h / 2], [w / 2, -h / 2], [w / 2, h / 2], [-w / 2, h / 2]])
        q = q @ np.array([[ca, sa], [-sa, ca]]) + [cx, cy] + rs.uniform(-3, 3, (4, 2))   # perspective jitter
        q = np.clip(np.round(q), [0, 0], [cols - 1, rows - 1]).astype(np.int32)
        if np.ptp(q[:, 0]) > 0 and np.ptp(q[:, 1]) > 0:
            out.append(q)
    return out


def test_rotate_crop_matches_oracle(pkg, built, card):
    """Utility::GetRotateCropImage (utility.cpp:137-190): homography in double on the host, warp on the device."""
    import oracle as O
    rs = np.random.RandomState(21)
    noise = rs.randint(0, 256, (300, 420, 3)).astype(np.uint8)
    for img in (card, noise, noise[20:280, 10:400]):              # the last one is a strided view
        rows, cols = img.shape[:2]
        quads = _random_quads(rs, rows, cols, 150)
        quads.append(np.array([[5, 7], [90, 7], [90, 40], [5, 40]], np.int32))          # axis-aligned: identity warp
        quads.append(np.array([[5, 7], [30, 7], [30, 140], [5, 140]], np.int32))        # tall: rot90 of the crop
        quads.append(np.array([[0, 0], [cols - 1, 0], [cols - 1, rows - 1], [0, rows - 1]], np.int32))
        quads.append(np.array([[50, 50], [50, 50], [80, 90], [50, 90]], np.int32))      # zero width -> dsize falls back
        got = pkg.rotate_crops(img, quads)
        for q, g in zip(quads, got):
            o = O.rotate_crop(img, q)
            assert g.shape == o.shape == pkg.rotate_crop_shape(rows, cols, q) + (3,)
            assert np.array_equal(g, o)
        assert np.array_equal(got[150], img[7:40, 5:90])
        assert np.array_equal(got[151], np.rot90(img[7:140, 5:30]))
    with pytest.raises(pkg.OcrError, match="no crop inside"):
        pkg.rotate_crops(card, [np.array([[5, 5], [5, 5], [5, 5], [5, 5]], np.int32)])
    with pytest.raises(pkg.OcrError, match="no crop inside"):
        pkg.rotate_crops(card, [np.array([[-3, 5], [50, 5], [50, 30], [-3, 30]], np.int32)])


def test_rotations_of_overlapping_rois_keep_request_order(pkg, built):
    """The classifier's in-place cv::rotate on ROI views of one image (ocr_worker.cpp:255-262): overlapping crops see
    each other's result, so the device's level schedule (disjoint ROIs concurrently, intersecting ones in list order)
    must equal rotating one after the other."""
    import oracle as O
    rs = np.random.RandomState(77)
    img = rs.randint(0, 256, (240, 330, 3)).astype(np.uint8)
    cases = []
    # chains of overlapping rectangles, nested ones, odd/even sizes, single rows/columns, repeats of the same rectangle
    cases.append([(10, 10, 100, 40), (60, 30, 120, 41), (150, 50, 51, 33), (10, 10, 100, 40), (0, 0, 330, 240)])
    cases.append([(5, 5, 1, 1), (5, 5, 2, 1), (5, 5, 1, 2), (7, 3, 9, 1), (3, 7, 1, 9), (0, 0, 3, 3)])
    cases.append([(x, y, 37, 21) for y in range(0, 200, 13) for x in range(0, 280, 29)])          # dense overlaps: many levels
    cases.append([(x, y, 20, 10) for y in range(0, 230, 10) for x in range(0, 320, 20)])          # a disjoint tiling: one level
    rnd = []
    for _ in range(200):
        w, h = rs.randint(1, 120), rs.randint(1, 60)
        rnd.append((rs.randint(0, 330 - w + 1), rs.randint(0, 240 - h + 1), w, h))
    cases.append(rnd)
    for rects in cases:
        want = img.copy()
        for (x, y, w, h) in rects:
            O.rotate180_inplace(want[y:y + h, x:x + w])
        got = pkg.rotate180_rois(img, rects)
        assert np.array_equal(got, want)
    # strided host image
    view = img[:, 10:300]
    want = np.ascontiguousarray(view).copy()
    for (x, y, w, h) in cases[0][:3]:
        O.rotate180_inplace(want[y:y + h, x:x + w])
    assert np.array_equal(pkg.rotate180_rois(view, cases[0][:3]), want)
    with pytest.raises(pkg.OcrError, match="outside the image"):
        pkg.rotate180_rois(img, [(300, 10, 40, 10)])


@pytest.mark.parametrize("cls_on", [False, True])
def test_pipeline_rotate_crop_mode(pkg, built, card, cls_on):
    """Opt-in crop mode: every det box goes through GetRotateCropImage instead of the ROI view."""
    from pipeline import Pipeline
    pg = pkg.Pipe(enable_cls=cls_on, crop_mode=pkg.CROP_ROTATE)
    po, pr = Pipeline(enable_cls=cls_on, crop_mode="rotate"), Pipeline(enable_cls=cls_on)
    imgs = [card, np.ascontiguousarray(np.rot90(card)), card[:120].copy()]
    got = pg.run(imgs)
    differs = 0
    for img, g in zip(imgs, got):
        w = po.process(img)["words"]
        assert len(g) == len(w) > 0
        for a, b in zip(g, w):
            assert np.array_equal(a["box"], b["box"]) and np.array_equal(a["ids"], b["ids"])
            assert a["confidence"] == np.float32(b["confidence"])
        # (the plain-mode answers for the card and its top strip are the ones test_pipeline_process_request asked for)
        cached = _ORACLE_CACHE.get(("process_request", cls_on))
        k = 0 if img is imgs[0] else 2 if img is imgs[2] else -1
        wr = cached[0][k] if cached and k >= 0 else pr.process(img)["words"]
        differs += sum(a["confidence"] != b["confidence"] for a, b in zip(w, wr))
    assert differs > 0      # the mode changes what rec sees
    pg.close()


def test_pipeline_device_resident_bench_protocol(pkg, built):
    import oracle as O
    from pipeline import Pipeline, DetCfg
    from synth_data import cfg2_sample
    s = [cfg2_sample(i) for i in range(2)]
    imgs, probs = np.stack([a[0] for a in s]), np.stack([a[1] for a in s])
    pg = pkg.Pipe(enable_cls=True, limit_side_len=960, rec_batch_num=16, rec_img_h=48, rec_img_w=320)
    d_i, d_p = pkg.DevArray(imgs), pkg.DevArray(probs)
    got = pg.run_device(d_i, 960, 960, 2, d_p)
    assert np.array_equal(d_i.download(), imgs)   # the caller's images are cloned, not rotated in place
    po = Pipeline(det_cfg=DetCfg(limit_side_len=960), rec_batch_num=16, rec_img_h=48, rec_img_w=320, enable_cls=True)
    for i in range(2):
        img = imgs[i].copy()
        boxes = O.det_post(probs[i], 0.2, 0.4, 1.8, 960, 960)
        views = [img[y:y + h, x:x + w] for x, y, w, h in (O.crop_rect(b, 960, 960) for b in boxes)]
        labels, _ = po.cls_run(views)
        for k, v in enumerate(views):
            if labels[k] == 1:
                O.rotate180_inplace(v)
        texts, scores, _ = po.rec_run(views)
        assert len(got[i]) == len(texts) == 32
        for k, g in enumerate(got[i]):
            assert np.array_equal(g["box"], boxes[k]) and np.array_equal(g["ids"], texts[k]) and g["confidence"] == scores[k]
    pg.close()


def test_pipeline_cfg3_mixed_sizes(pkg, built):
    """cfg3: images of different sizes in one call (each size its own det pass, 'max' limit 960 rounds to
    multiples of 32), cls on, whole path through the real networks (synthetic det/rec weights)."""
    from pipeline import Pipeline, DetCfg
    from synth_data import cfg3_sample
    imgs = [cfg3_sample(i)[0] for i in range(3)]
    assert len({im.shape for im in imgs}) == 3
    kw = dict(rec_batch_num=16, rec_img_h=48, rec_img_w=320, enable_cls=True)
    pg = pkg.Pipe(limit_side_len=960, **kw)
    po = Pipeline(det_cfg=DetCfg(limit_side_len=960), **kw)
    got = pg.run(imgs + [imgs[0]])                       # a repeated size shares its det pass
    pg1 = pkg.Pipe(limit_side_len=960, phases=1, **kw)   # one chain: word for word what the two chains gave
    got1 = pg1.run(imgs + [imgs[0]])
    assert [len(g) for g in got1] == [len(g) for g in got]
    assert all(np.array_equal(a["box"], b["box"]) and np.array_equal(a["ids"], b["ids"]) and a["confidence"] == b["confidence"]
               for ga, gb in zip(got, got1) for a, b in zip(ga, gb))
    pg1.close()
    for img, g in zip(imgs + [imgs[0]], got):
        nr, nc = pg.det_shape(*img.shape[:2])
        assert nr % 32 == 0 and nc % 32 == 0 and max(nr, nc) <= 960
        w = po.process(img)["words"]
        assert len(g) == len(w)
        for a, b in zip(g, w):
            assert np.array_equal(a["box"], b["box"]) and np.array_equal(a["ids"], b["ids"])
            assert a["confidence"] == np.float32(b["confidence"])
    assert sum(len(g) for g in got) > 0
    assert all(np.array_equal(a["box"], b["box"]) and np.array_equal(a["ids"], b["ids"]) for a, b in zip(got[0], got[3]))
    pg.close()


@pytest.mark.parametrize("mode", ["std", "stable"])
def test_rec_batches_with_tied_ratios_follow_the_sort_mode(pkg, built, mode):
    """More than rec_batch_num crops with EQUAL w/h ratios: which of them share a batch (and so its tensor width)
    depends on how std::sort orders ties (Utility::argsort, utility.cpp:192-203).  Both orders are available
    (ocr_rec_cfg.sort_mode); each must equal the oracle run in the same mode, ids, scores and per-step taps."""
    from pipeline import Pipeline
    rs = np.random.RandomState(31)
    crops = []
    for i in range(40):   # three ratio classes, 40 crops: ties straddle the batch boundaries at 16 and 32
        h, w = [(24, 96), (12, 48), (30, 200)][i % 3] if i % 5 else (20, 300 + i)
        crops.append(rs.randint(0, 255, (h, w, 3)).astype(np.uint8))
    pipe = Pipeline(rec_batch_num=16, rec_img_h=48, rec_img_w=320, rec_sort=mode)
    rec = pkg.Rec(rec_batch_num=16, rec_img_h=48, rec_img_w=320, sort_mode=1 if mode == "stable" else 0)
    to, so, steps = pipe.rec_run(crops)
    tg, sg = rec.run(crops)
    for i in range(len(crops)):
        assert np.array_equal(to[i], tg[i]), i
        assert so[i] == sg[i], i
        am, pm = rec.steps(i)
        assert np.array_equal(am, steps[i][0]) and np.array_equal(pm, steps[i][1]), i
    rec.close()


def test_pipeline_production_batch_equals_oracle_on_sampled_images(pkg, built):
    """BASELINE configs[1] at its full size: 64 synthetic 960x960 images (2048 text lines) in one call - the batch at
    which the production-only paths switch on (workgroups with several units in the fused depthwise->pointwise kernels,
    depthwise convs that leave the pool's row sums, the 1872-line rec launch beside the small-width lanes, 64-image det
    tensors of 0.9 GB).  Results are batch-invariant, so any image's words must equal what the oracle produces for that
    image alone: checked on five images spread over the batch (the oracle needs ~2 s per image)."""
    from pipeline import Pipeline, DetCfg
    from synth_data import cfg2_sample
    kw = dict(rec_batch_num=16, rec_img_h=48, rec_img_w=320, enable_cls=True)
    pg = pkg.Pipe(limit_side_len=960, **kw)
    po = Pipeline(det_cfg=DetCfg(limit_side_len=960), **kw)
    samples = [cfg2_sample(i) for i in range(64)]
    imgs = [s_[0] for s_ in samples]
    probs = [s_[1] for s_ in samples]
    pg.stage(0, imgs, probs)
    got = pg.run_staged(0)
    assert len(got) == 64 and sum(len(g) for g in got) == 64 * 32
    for i in (0, 13, 31, 46, 63):
        w = po.process(imgs[i], probs[i])["words"]
        assert len(got[i]) == len(w) == 32, i
        for a, b in zip(got[i], w):
            assert np.array_equal(a["box"], b["box"]) and np.array_equal(a["ids"], b["ids"]), i
            assert a["confidence"] == np.float32(b["confidence"]), i
    pg.close()
    # the detection network itself at 64 images per launch (the pipeline above thresholds the protocol's synthetic maps):
    # probability maps of two images far into the batch against the oracle's
    det = pkg.Det(limit_side_len=960, thresh=0.3, box_thresh=0.5, unclip_ratio=2.0, max_batch=64)
    det.run_batch(imgs)
    for i in (41, 63):
        po.det_run(imgs[i])
        assert np.array_equal(det.prob_map(i), po.taps["det_prob"]), i
    det.close()


def test_pipeline_cfg3_pooled_lines_and_staged_slots(pkg, built):
    """BASELINE configs[2] shape of work: 16 images of 16 distinct sizes in ONE call.  det runs per size; the text
    lines of all images share one cls pass and one rec pass (pipe.hip run_images) - every word must still equal
    what the oracle produces for that image alone.  Synthetic probability maps (SURVEY 8d protocol) so that every
    image has lines.  Also: the double-buffered staging API - slot 1 staged while slot 0's results are read, a slot
    run twice gives the same words (the staged images are not rotated in place), run() == stage + run_staged."""
    from pipeline import Pipeline, DetCfg
    from synth_data import cfg3_sample, cfg3_prob_at
    kw = dict(rec_batch_num=16, rec_img_h=48, rec_img_w=320, enable_cls=True)
    pg = pkg.Pipe(limit_side_len=960, **kw)
    po = Pipeline(det_cfg=DetCfg(limit_side_len=960), **kw)
    imgs = [cfg3_sample(i)[0] for i in range(16)]
    assert len({im.shape for im in imgs}) >= 8
    probs = [cfg3_prob_at(i, *pg.det_shape(*imgs[i].shape[:2])) for i in range(16)]
    pg.stage(0, imgs[:10], probs[:10])
    pg.stage(1, imgs[10:], probs[10:])
    got = pg.run_staged(0) + pg.run_staged(1)
    again = pg.run_staged(0)
    total = 0
    for i, g in enumerate(got):
        w = po.process(imgs[i], probs[i])["words"]
        assert len(g) == len(w) > 0, i
        total += len(g)
        for a, b in zip(g, w):
            assert np.array_equal(a["box"], b["box"]) and np.array_equal(a["ids"], b["ids"])
            assert a["confidence"] == np.float32(b["confidence"])
    assert total > 200
    for a, b in zip(again, got[:10]):
        assert len(a) == len(b) and all(np.array_equal(x["ids"], y["ids"]) and x["confidence"] == y["confidence"] for x, y in zip(a, b))
    pg.close()


def _cfg3_pool_item(i):
    from synth_data import cfg3_item
    return cfg3_item(i)


@pytest.mark.timeout(900)
def test_pipeline_configs2_full_size_with_binding_eviction_and_changing_slots(pkg, built, monkeypatch):
    """BASELINE configs[2] at its full size: 512 mixed 640-1280 px images (>= 300 distinct detector shapes) in ONE call,
    with the networks' binding caches capped at 16 shapes so that every detector lane keeps evicting and re-binding
    (the 512-entry LRU of production is never under pressure in the small tests).  Eight sampled images are checked
    word for word against the oracle; then the same images go through the two staging slots in batches of 64 with a
    NEW composition every time (the request-stream path of configs[3]) and every image's words must equal what the
    full batch gave for it - results do not depend on what else is in a batch."""
    import multiprocessing as mp
    from pipeline import Pipeline, DetCfg
    n = 512
    with mp.get_context("spawn").Pool(12) as pool:       # (spawned: this process has initialised the GPU)
        items = pool.map(_cfg3_pool_item, range(n), chunksize=8)
    imgs, probs = [it[0] for it in items], [it[1] for it in items]
    assert len({im.shape for im in imgs}) >= 300
    kw = dict(rec_batch_num=16, rec_img_h=48, rec_img_w=320, enable_cls=True)
    pg = pkg.Pipe(limit_side_len=960, **kw)       # default: the detector runs the mixed sizes as ragged launches (one per ~64 Mpixel)
    for i in (0, 100, 511):
        assert pg.det_shape(*imgs[i].shape[:2]) == probs[i].shape
    pg.stage(0, imgs, probs)
    got = pg.run_staged(0)
    same = lambda a, b: len(a) == len(b) and all(np.array_equal(x["box"], y["box"]) and np.array_equal(x["ids"], y["ids"]) and
                                                 x["confidence"] == y["confidence"] for x, y in zip(a, b))
    assert sum(len(g) for g in got) > 10000
    # the per-size path of rounds 1-2 (one detector pass per distinct size on the lanes), with the binding caches capped
    # at 16 shapes: every lane keeps evicting and re-binding; all 512 images must give the ragged launches' words
    monkeypatch.setenv("OCR_NET_BINDINGS", "16")
    monkeypatch.setenv("OCR_DET_RAGGED", "0")
    pl = pkg.Pipe(limit_side_len=960, **kw)
    monkeypatch.delenv("OCR_NET_BINDINGS")
    monkeypatch.delenv("OCR_DET_RAGGED")
    st0 = pl.stats()
    pl.stage(0, imgs, probs)
    lanes = pl.run_staged(0)
    st1 = pl.stats()
    assert st1["binds"] - st0["binds"] >= 300                       # one per distinct shape at least
    again = pl.run_staged(0)                                         # the capped caches re-bind what they evicted
    assert pl.stats()["binds"] - st1["binds"] >= 100
    assert all(same(a, b) for a, b in zip(lanes, again))
    assert all(same(a, b) for a, b in zip(lanes, got))
    pl.close()
    po = Pipeline(det_cfg=DetCfg(limit_side_len=960), **kw)
    for i in (0, 63, 64, 200, 255, 256, 400, 511):
        w = po.process(imgs[i], probs[i])["words"]
        assert len(got[i]) == len(w) > 0, i
        for a, b in zip(got[i], w):
            assert np.array_equal(a["box"], b["box"]) and np.array_equal(a["ids"], b["ids"]) and a["confidence"] == np.float32(b["confidence"])
    # the stream path: alternating slots, a new composition of 64 images every batch (strided picks: sizes mix differently)
    rs = np.random.RandomState(9)
    for b in range(6):
        ids = rs.permutation(n)[:64]
        pg.stage(b & 1, [imgs[i] for i in ids], [probs[i] for i in ids])
        out = pg.run_staged(b & 1)
        assert all(same(out[k], got[i]) for k, i in enumerate(ids)), b
    pg.close()
