"""The layer above the server kernels (BASELINE configs[4]): a request batch of MIXED image sizes through a pipeline whose
detector and recognizer are the server networks, and recognizer calls that are cut into several network launches.

Mixed sizes.  Four images of three sizes in one call, sizes interleaved (224x320, 320x224, 224x320, 192x320; limit_side_len 320,
so the detector's input is the image's own size): a size group of two images whose members are not neighbours in the request,
and, with the two chains of a pipeline, one chain with two size groups and one with a single group.  A server detector has no
ragged launch list: the pipeline runs its size groups one after another on the chain's one detector (pipe.hip, run_images).
Boxes come from the section-8d probability maps (synth_data.cfg2_sample), attached to slot 0 with Pipe.stage - Pipe.run re-stages
the same layout and keeps them.  The sizes are the smallest at which the four images give 20 lines or more (the layouts hold
lines 80 px wide and up: 160x224 and 96x320 give two or three lines an image), so that the 90 % floor of the fp16 comparison
is a statement about more than a dozen lines.

Launch cuts.  ocr_rec_set_launch_lines (a self-test entry point) lowers RecStage::max_lines_per_launch, so that seven lines run
as 3 + 3 + 1 and as seven launches of the server recognizer, and as budget-cut ragged launches of the mobile one: every result
of the call - ids, lengths, scores, per-character steps / run lengths / confidences, top-k ids and probabilities, the step taps
and the tapped logits rows - equals the uncut call's bit for bit.

Tile tuning is timed per new (layer, shape) and would dominate: every server case runs in a child process with OCR_SRV_TUNE=0
(read once per process), at most four children at a time, started together so that they overlap the oracle's CPU run of the four
images.  The children keep the suite's tuning file, so launches of different batch sizes do run on different tiles; every tile
configuration gives the same bits (logits: test_every_tile_configuration_gives_the_same_bits; the f16 head's CTC partials: the
forced-tile children here)."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "cpp-paddle-ocr_amd", "host")
SRV = os.path.join(ROOT, "models_server")
KEYS = os.path.join(ROOT, "models", "rec", "ppocr_keys_v1.txt")
OCR_ERR_ARG = -1

# ------------------------------------------------------------------------------------------ inputs
MIXED = [(224, 320, 100), (320, 224, 101), (224, 320, 102), (192, 320, 101)]  # rows, cols, cfg2 sample: request order
LIMIT = 320
PIPE_KW = dict(enable_cls=True, limit_side_len=LIMIT, rec_batch_num=16, rec_img_h=48, rec_img_w=320)


def mixed_inputs():
    from synth_data import cfg2_sample
    samples = [cfg2_sample(i, h, w, 8) for h, w, i in MIXED]
    return [s[0] for s in samples], [s[1] for s in samples]


def cut_crops():
    """seven lines 48 px high; with batches of two (sorted by w / h) the mobile tensor widths are 320, 320, 380, 380, 480, 480, 640"""
    rs = np.random.RandomState(77)
    widths = [480, 100, 640, 400, 320, 200, 380]  # input order is not width order
    return [rs.randint(0, 256, (48, w, 3)).astype(np.uint8) for w in widths]


# ------------------------------------------------------------------------------------------ what a child prints
def _f32_bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32).tolist()


def _words_json(per_image):
    return [[dict(box=w["box"].ravel().tolist(), ids=w["ids"].tolist(), conf=_f32_bits([w["confidence"]])[0]) for w in ws] for ws in per_image]


def _conf(word):
    return float(np.array([word["conf"]], np.uint32).view(np.float32)[0])


def snapshot(rec, crops):
    """every result a recognizer call has, in JSON terms (floats as their bits, logits rows as digests)"""
    ids, scores = rec.run(crops)
    out = dict(ids=[t.tolist() for t in ids], lens=[len(t) for t in ids], scores=_f32_bits(scores))
    ids3, scores3, chars = rec.run_chars(crops, topk=3)
    out["chars_ids"] = [t.tolist() for t in ids3]
    out["chars_scores"] = _f32_bits(scores3)
    out["steps"] = [c["steps"].tolist() for c in chars]
    out["nsteps"] = [c["nsteps"].tolist() for c in chars]
    out["probs"] = [_f32_bits(c["probs"]) for c in chars]
    out["geom"] = [list(c["geom"]) for c in chars]
    out["alt_ids"] = [c["alt_ids"].ravel().tolist() for c in chars]
    out["alt_probs"] = [_f32_bits(c["alt_probs"].ravel()) for c in chars]
    out["tap_amax"], out["tap_pmax"], out["rows"] = [], [], []
    for i, c in enumerate(chars):
        am, pm = rec.steps(i, cap=8192)
        out["tap_amax"].append(am.tolist())
        out["tap_pmax"].append(_f32_bits(pm))
        T = len(am)
        picked = sorted({0, T // 2, T - 1} | set(int(s) for s in c["steps"][:4]))
        rows = [rec.logits_row(i, s) for s in picked]
        assert all(int(np.argmax(r)) == int(am[s]) for r, s in zip(rows, picked)), i  # the row of THIS line's step
        out["rows"].append([hashlib.sha1(r.tobytes()).hexdigest() for r in rows])
    return out


RESULT_KEYS = ("ids", "lens", "scores", "chars_ids", "chars_scores", "steps", "nsteps", "probs", "geom", "alt_ids", "alt_probs",
               "tap_amax", "tap_pmax", "rows")


def assert_same_call(cut, whole, what):
    for k in RESULT_KEYS:
        assert cut[k] == whole[k], (what, k)
    # the comparison means something: the lines differ from each other, first tapped row (step 0) included
    assert len({r[0] for r in whole["rows"]}) == len(whole["rows"]), what
    assert sum(whole["lens"]) > 0, what


def _network_runs(report):
    """network runs since timing was switched on: every run of the server network starts with its one pack_input launch"""
    return report["pack_input"]["count"] if "pack_input" in report else 0


# ------------------------------------------------------------------------------------------ children
def _pipe_child(mode):
    import __graft_entry__ as ge
    pkg = ge.load_package()
    imgs, probs = mixed_inputs()
    out = {}
    for prec in ("fp32", "fp16"):
        pipe = pkg.Pipe(device=0, precision=prec, det_dir=os.path.join(SRV, "det"), rec_dir=os.path.join(SRV, "rec"), **PIPE_KW)
        r = out[prec] = {}
        pipe.stage(0, imgs, probs)
        pipe.timing(True)
        try:
            r["mixed"] = _words_json(pipe.run(imgs))
        except pkg.OcrError as e:  # (reported, not raised: the parent says what failed)
            r["error"] = str(e)
            pipe.close()
            continue
        rep = pipe.timing_report()
        pipe.timing(False)
        r["det_runs"] = _network_runs({k[4:]: v for k, v in rep.items() if k.startswith("det.")})
        r["rec_runs"] = _network_runs({k[4:]: v for k, v in rep.items() if k.startswith("rec.")})
        r["det_counts"] = sorted({v["count"] for k, v in rep.items() if k.startswith("det.") and k != "det.pack_input"})
        if mode == "full":
            pipe.stage(1, imgs, probs)
            r["staged"] = _words_json(pipe.run_staged(1))
            r["alone"] = []
            for im, pr in zip(imgs, probs):
                pipe.stage(0, [im], [pr])
                r["alone"].append(_words_json(pipe.run([im]))[0])
            pipe.stage(0, imgs, probs)
            r["again"] = _words_json(pipe.run(imgs))  # after other shapes went through the same detector and recognizer
        pipe.close()
    return out


def _rec_child(mode):
    import __graft_entry__ as ge
    pkg = ge.load_package()
    crops = cut_crops()
    out = {}
    for prec in ("fp16",) if mode == "tile" else ("fp32", "fp16"):
        rec = pkg.Rec(model_dir=os.path.join(SRV, "rec"), label_path=KEYS, rec_batch_num=16, rec_img_h=48, rec_img_w=320, precision=prec)
        r = out[prec] = dict(whole=snapshot(rec, crops))
        if mode == "tile":  # a forced tile configuration (OCR_SRV_CFG): the uncut call, one launch of seven and one of three, and the head's tile
            rec.set_launch_lines(3)
            rec.timing(True)
            rec.run(crops)
            r["head"] = sorted(k for k in rec.timing_report() if "_ctc[" in k)
            r["cut3"] = snapshot(rec, crops)
            rec.close()
            continue
        try:
            rec.set_launch_lines(0)
            r["bad"] = "accepted"
        except pkg.OcrError as e:
            r["bad"] = str(e)
        r["after_bad"] = snapshot(rec, crops)
        for n in (3, 1):
            rec.set_launch_lines(n)
            rec.timing(True)
            rec.run(crops)
            runs = [_network_runs(rec.timing_report())]
            rec.timing(True)
            rec.run_chars(crops, topk=3)
            runs.append(_network_runs(rec.timing_report()))
            rec.timing(False)
            r["cut%d" % n] = snapshot(rec, crops)
            r["runs%d" % n] = runs
        rec.set_launch_lines(4096)
        r["back"] = snapshot(rec, crops)
        rec.close()
    return out


_CHILD = r"""
import json, sys
sys.path[:0] = [sys.argv[1], sys.argv[1] + "/tools", sys.argv[1] + "/oracle", sys.argv[1] + "/tests"]
import test_gpu_srv_pipeline as T
print("CHILD " + json.dumps(getattr(T, sys.argv[2])(sys.argv[3])))
"""
CHILDREN = {
    "default": ("_pipe_child", "full", {}),
    "ragged0": ("_pipe_child", "mixed", {"OCR_DET_RAGGED": "0"}),
    "lanes1": ("_pipe_child", "mixed", {"OCR_DET_LANES": "1"}),
    "lanes8": ("_pipe_child", "mixed", {"OCR_DET_LANES": "8"}),
    "rec": ("_rec_child", "-", {}),
    # OCR_SRV_CFG forces a tile configuration on every GEMM that takes it (srv_net.hip, tune): 128x128/2x2, 256x256/2x4, 128x256/1x8,
    # 128x192/2x2 and 64x64/2x2 - one, two, three and four 32-column blocks per wave, one to eight waves per row, 64 to 256 columns
    "tile1": ("_rec_child", "tile", {"OCR_SRV_CFG": "1"}),
    "tile12": ("_rec_child", "tile", {"OCR_SRV_CFG": "12"}),
    "tile4": ("_rec_child", "tile", {"OCR_SRV_CFG": "4"}),
    "tile21": ("_rec_child", "tile", {"OCR_SRV_CFG": "21"}),
    "tile9": ("_rec_child", "tile", {"OCR_SRV_CFG": "9"}),
}
TILES = {"tile1": "[128x128/2x2/", "tile12": "[256x256/2x4/", "tile4": "[128x256/1x8/", "tile21": "[128x192/2x2/", "tile9": "[64x64/2x2/"}
FATAL = (-6, -11, -9, 134, 139, 124, 137)  # abort, segmentation fault, kill / time limit: nothing more is started on the card after one


class _Children:
    """the child processes, at most four at a time; a result is waited for where a test first asks for it"""

    def __init__(self):
        self.pending, self.running, self.done, self.stopped = list(CHILDREN), {}, {}, None
        self._fill()

    def _fill(self):
        while self.pending and len(self.running) < 4 and self.stopped is None:
            name = self.pending.pop(0)
            fn, mode, env = CHILDREN[name]
            env = dict(os.environ, OCR_SRV_TUNE="0", **env)
            # (the suite's tuning file, conftest.py, stays: it goes before OCR_SRV_TUNE=0 in SrvNet::tune and holds timed tiles for SOME
            # batch sizes - the comparisons below hold across whatever mix of tiles that gives)
            for k in ("OCR_DET_RAGGED", "OCR_DET_LANES", "OCR_SRV_CFG"):
                if k not in CHILDREN[name][2]:
                    env.pop(k, None)
            self.running[name] = subprocess.Popen([sys.executable, "-c", _CHILD, ROOT, fn, mode], env=env, stdout=subprocess.PIPE,
                                                  stderr=subprocess.PIPE, text=True)

    def close(self):
        """the children no test asked for: reaped (killed if they have not ended)"""
        for pr in self.running.values():
            if pr.poll() is None:
                pr.kill()
            pr.communicate()
        self.running.clear()

    def get(self, name):
        while name not in self.done:
            assert self.running, "child %s was not started: child %s ended with %s" % (name, *(self.stopped or ("?", "?")))
            first = name if name in self.running else next(iter(self.running))
            pr = self.running.pop(first)
            try:
                so, se = pr.communicate(timeout=600)
            except subprocess.TimeoutExpired:
                pr.kill()
                so, se = pr.communicate()
                se += "\nTIMEOUT"
            self.done[first] = (pr.returncode, so, se)
            if pr.returncode in FATAL or "TIMEOUT" in se[-10:]:
                self.stopped = self.stopped or (first, pr.returncode)
            self._fill()
        rc, so, se = self.done[name]
        assert rc == 0 and "CHILD " in so, (name, rc, so[-2000:], se[-3000:])
        return json.loads(so[so.index("CHILD ") + 6:].splitlines()[0])


@pytest.fixture(scope="module")
def children(built):
    import synth_weights
    synth_weights.ensure_server(ROOT)
    ch = _Children()
    yield ch
    ch.close()


@pytest.fixture(scope="module")
def oracle_words(children):
    """the oracle pipeline's words of the four images, each processed alone (the children are running meanwhile)"""
    import pipeline as P
    imgs, probs = mixed_inputs()
    ora = P.Pipeline(P.DetCfg(limit_side_len=LIMIT), rec_batch_num=16, rec_img_h=48, rec_img_w=320, enable_cls=True, det_net="srv_det",
                     rec_net="srv_rec")
    want = [ora.process(im, prob_override=pr)["words"] for im, pr in zip(imgs, probs)]
    assert all(len(w) >= 2 for w in want), [len(w) for w in want]
    assert sum(len(w) for w in want) >= 20, [len(w) for w in want]
    return want


def _mixed(children, name, prec):
    r = children.get(name)[prec]
    assert "error" not in r, (name, prec, r.get("error"))
    return r


# ------------------------------------------------------------------------------------------ mixed sizes
def test_mixed_sizes_fp32_twin_equals_the_oracle(children, oracle_words):
    """boxes and CTC ids exactly, confidences to the 1e-5 of the single-size twin test (the device sums the softmax in its own
    order); image i of the answer is image i of the request"""
    got = _mixed(children, "default", "fp32")["mixed"]
    assert len(got) == len(oracle_words) == 4
    for i, (g, w) in enumerate(zip(got, oracle_words)):
        assert len(g) == len(w), (i, len(g), len(w))
        for a, b in zip(g, w):
            assert a["box"] == np.array(b["box"]).ravel().tolist(), i
            assert a["ids"] == list(b["ids"]), i
            assert abs(_conf(a) - b["confidence"]) <= 1e-5, (i, _conf(a), b["confidence"])
    # request order is visible: the two 224 x 320 images (0 and 2) have different words, and so have the neighbours in layout order
    assert [w["box"] for w in got[0]] != [w["box"] for w in got[2]]


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
def test_mixed_call_equals_each_image_alone_and_the_staged_path(children, prec):
    """bit for bit, confidences included: through the same handle each image alone, the same batch staged with its maps
    (Pipe.stage + run_staged), and the mixed call once more after those other shapes"""
    r = _mixed(children, "default", prec)
    assert r["mixed"] == r["alone"]
    assert r["mixed"] == r["staged"]
    assert r["mixed"] == r["again"]
    assert sum(len(ws) for ws in r["mixed"]) >= 20


def test_mixed_sizes_fp16_boxes_equal_the_oracle_and_ids_stay_close(children, oracle_words):
    """fp16 (the mode configs[4] names): the boxes are the oracle's (known maps), and at least 90 % of the lines have the
    oracle's id sequence - the floor of the single-size test, here over 20 lines or more"""
    got = _mixed(children, "default", "fp16")["mixed"]
    lines = same = 0
    for i, (g, w) in enumerate(zip(got, oracle_words)):
        assert len(g) == len(w), (i, len(g), len(w))
        for a, b in zip(g, w):
            assert a["box"] == np.array(b["box"]).ravel().tolist(), i
            lines += 1
            same += a["ids"] == list(b["ids"])
    print("server pipeline, mixed sizes, fp16: %d of %d lines have the oracle's id sequence" % (same, lines))
    assert lines >= 20
    assert same >= 0.9 * lines, (same, lines)


@pytest.mark.parametrize("name", ["ragged0", "lanes1", "lanes8"])
@pytest.mark.parametrize("prec", ["fp32", "fp16"])
def test_detector_switches_do_not_change_the_words(children, name, prec):
    """OCR_DET_RAGGED=0, OCR_DET_LANES=1 and =8: a server detector takes one pass per size group under each of them"""
    assert _mixed(children, name, prec)["mixed"] == _mixed(children, "default", prec)["mixed"]
    assert _mixed(children, name, prec)["det_runs"] == 3


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
def test_one_detector_pass_per_size_group_on_the_chains_own_detector(children, prec):
    """the timing report of the default run: three runs of the server detector - one per size group, two on one chain and one
    on the other - every launch name once (a name carries its shape), and a recognizer run per chain.  A further detector
    instance is not in the report (pipe_srv_nets): its runs would be missing from the three."""
    r = _mixed(children, "default", prec)
    assert r["det_runs"] == 3, r["det_runs"]
    assert r["det_counts"] == [1], r["det_counts"]
    assert r["rec_runs"] == 2, r["rec_runs"]


# ------------------------------------------------------------------------------------------ launch cuts: server
@pytest.mark.parametrize("prec", ["fp32", "fp16"])
def test_server_recognizer_cut_into_launches_equals_the_uncut_call(children, prec):
    """seven lines as 3 + 3 + 1 and as seven launches (LinesCtx::run_srv: step_off per slot, x_ reused, the network re-bound to
    another N, logits read from the network's output tensor before the next launch overwrites it) against one launch of seven"""
    r = children.get("rec")[prec]
    whole = r["whole"]
    assert all(g[:2] == [80, 320] for g in whole["geom"])
    assert_same_call(r["cut3"], whole, "3 + 3 + 1")
    assert_same_call(r["cut1"], whole, "seven launches")
    assert_same_call(r["back"], whole, "one launch again")
    assert r["runs3"] == [3, 3], r["runs3"]  # run, run_chars(topk=3)
    assert r["runs1"] == [7, 7], r["runs1"]


@pytest.mark.parametrize("name", list(TILES))
def test_fp16_server_results_do_not_depend_on_the_tile_configuration(children, name):
    """the f16 CTC head leaves softmax partials, not logits (srv_kernels.hip, ctc_part): a partial per 64 columns, formed in one order
    whatever the tile, so that a line's confidence does not depend on the tile tune() picked for the launch's batch size - which
    it did while a partial spanned the tile's columns.  Five forced tiles against the default child's choice: every result of the
    uncut call and of the 3 + 3 + 1 cut, bit for bit (the top-k call's logits path included)"""
    r = children.get(name)["fp16"]
    assert r["head"] and all(TILES[name] in k for k in r["head"]), r["head"]  # the head did run on the forced tile
    want = children.get("rec")["fp16"]["whole"]
    assert_same_call(r["whole"], want, name)
    assert_same_call(r["cut3"], want, name + ", 3 + 3 + 1")


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
def test_server_recognizer_refuses_zero_lines_per_launch(children, prec):
    r = children.get("rec")[prec]
    assert "error %d" % OCR_ERR_ARG in r["bad"] and "lines per launch" in r["bad"], r["bad"]
    assert_same_call(r["after_bad"], r["whole"], "after the refusal")


# ------------------------------------------------------------------------------------------ launch cuts: mobile
@pytest.fixture(scope="module")
def plan_check(tmp_path_factory):
    exe = os.path.join(str(tmp_path_factory.mktemp("recplan")), "rec_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-o", exe, os.path.join(HOST, "rec_plan_check.cpp")])
    return exe


def planned_slots(exe, crops, cap, batch_num, tmp_path):
    """(tensor widths in launch order, slots) of a call, by the header RecStage::run_lines runs (host/rec_plan_check.cpp)"""
    from rec_plan_cases import Case, parse
    case = Case([(c.shape[1], c.shape[0]) for c in crops], batch_num=batch_num, cap=cap)
    path = os.path.join(str(tmp_path), "case_%d.txt" % cap)
    with open(path, "w") as f:
        f.write(case.text() + "\n")
    kind, items, slots = parse(subprocess.run([exe, path], capture_output=True, text=True, check=True).stdout, 1)[0]
    assert kind == "plan"
    return [it[2] for it in items], slots


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
def test_mobile_recognizer_budget_cut_ragged_launches_equal_the_uncut_call(pkg, built, plan_check, tmp_path, prec):
    """lines-per-launch 3 is a budget of 960 tensor columns: 320 + 320 | 380 + 380 | 480 + 480 | 640, four ragged launches; 1 is
    seven of them (every line alone is past 320 columns or fills them)"""
    crops = cut_crops()
    widths, slots = planned_slots(plan_check, crops, 3, 2, tmp_path)
    assert widths == [320, 320, 380, 380, 480, 480, 640]
    assert slots == [(0, 2, 1), (2, 2, 1), (4, 2, 1), (6, 1, 1)]
    assert planned_slots(plan_check, crops, 1, 2, tmp_path)[1] == [(i, 1, 1) for i in range(7)]
    assert planned_slots(plan_check, crops, 4096, 2, tmp_path)[1] == [(0, 7, 1)]
    rec = pkg.Rec(rec_batch_num=2, rec_img_h=48, rec_img_w=320, precision=prec)
    whole = snapshot(rec, crops)
    assert sorted(g[1] for g in whole["geom"]) == widths
    with pytest.raises(pkg.OcrError, match="lines per launch"):
        rec.set_launch_lines(0)
    assert_same_call(snapshot(rec, crops), whole, "after the refusal")
    for n in (3, 1):
        rec.set_launch_lines(n)
        assert_same_call(snapshot(rec, crops), whole, "lines per launch %d" % n)
    rec.close()
    if prec == "fp32":
        from pipeline import Pipeline
        to, so, steps = Pipeline(rec_batch_num=2, rec_img_h=48, rec_img_w=320).rec_run(crops)
        assert whole["ids"] == [list(t) for t in to]
        assert whole["scores"] == _f32_bits(so)


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
def test_mobile_uniform_launches_behind_budget_cut_ragged_ones(pkg, built, plan_check, tmp_path, prec):
    """two lines wider than the ragged attention kernel takes, in the middle of the request: launches go in ascending tensor
    width, so they are uniform launches behind the budget-cut ragged ones - ragged | ragged | ragged | ragged | uniform | uniform,
    the first uniform launch with launches (and non-zero step offsets) on both sides"""
    bound = int(subprocess.run([plan_check, "--ragged-bound"], capture_output=True, text=True, check=True).stdout)
    rs = np.random.RandomState(78)
    seven = cut_crops()
    wide = [rs.randint(0, 256, (48, w, 3)).astype(np.uint8) for w in (bound + 104, bound)]
    crops = seven[:3] + [wide[0]] + seven[3:5] + [wide[1]] + seven[5:]
    widths, slots = planned_slots(plan_check, crops, 3, 1, tmp_path)
    assert widths == [320, 320, 320, 380, 400, 480, 640, bound, bound + 104]
    assert slots == [(0, 3, 1), (3, 2, 1), (5, 1, 1), (6, 1, 1), (7, 1, 0), (8, 1, 0)]
    rec = pkg.Rec(rec_batch_num=1, rec_img_h=48, rec_img_w=320, precision=prec)
    whole = snapshot(rec, crops)  # (uncut: one ragged launch and the two uniform ones)
    rec.set_launch_lines(3)
    assert_same_call(snapshot(rec, crops), whole, "ragged x 4, uniform x 2")
    rec.close()
