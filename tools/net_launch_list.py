"""What Net::bind decided, as seen from outside: per case the launch list (name, count, algorithmic flops and bytes of every
launch of one forward, from the per-launch timing report) and which plan tensors the binding writes to device memory.

Meant for refactors of the binder: record the output at the commit before (on the GPU), run it again after, and a moved
fusion decision, launch name or flops / bytes formula shows up as a diff of two lists.

    python tools/net_launch_list.py [--group main|switch] [--out FILE]

Uses only binding.Net / binding.Pipe: timing(True), one forward, timing_report(), exists(tid)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

UNIFORM = [("cls", (3, 48, 192)), ("det", (2, 96, 160)), ("det", (3, 64, 64)), ("rec", (3, 48, 320)), ("rec", (2, 28, 192))]
RAGGED_REC = (48, [320, 327, 40, 1000, 64])
RAGGED_DET = [(96, 160), (32, 32), (64, 224), (160, 96)]
# runtime switches that change decisions on these small shapes; read once per process, so each set runs in a child process
CHILD_TIMEOUT_S = 120
SWITCHES = {"gap_min1_mt2_force": {"OCR_FUSE_GAP_MIN": "1", "OCR_CONV_MT2": "force"}, "fuse0": {"OCR_FUSE": "0"}}


def _pkg():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from __graft_entry__ import load_package
    return load_package()


def _rows(report):
    # (the report prints flops and bytes with %.0f: float() of that text and int() of the float are both exact, whatever the size)
    return sorted([name, r["count"], int(r["flops"]), int(r["bytes"])] for name, r in report.items())


def _net_case(pkg, net, forward):
    """one forward of `net` with per-launch timing on -> {"launches", "exists"}, or {"error"} when the forward is refused"""
    net.timing(True)
    try:
        forward()
    except pkg.OcrError as e:
        return {"error": str(e)}
    return {"launches": _rows(net.timing_report()),
            "exists": "".join("1" if net.exists(t) else "0" for t in range(net.num_tensors()))}


def uniform_cases(pkg, kinds=("cls", "det", "rec")):
    import numpy as np
    out = {}
    for precision in ("fp32", "fp16"):
        for kind, shape in UNIFORM:
            if kind not in kinds:
                continue
            x = np.random.RandomState(7).randn(shape[0], shape[1], shape[2], 3).astype(np.float32)
            keys = ["%s-%dx%dx%d-%s-keep%d" % ((kind,) + shape + (precision, k)) for k in (0, 1, 2)]
            try:
                net = pkg.Net(kind, precision=precision)
            except pkg.OcrError as e:  # the build refuses this network in this precision: noted, not fatal
                out.update({key: {"error": str(e)} for key in keys})
                continue
            for keep_all, key in enumerate(keys):
                out[key] = _net_case(pkg, net, lambda: net.forward(x, keep_all=keep_all))
            net.close()
    return out


def ragged_cases(pkg):
    import numpy as np
    rs = np.random.RandomState(8)
    out = {}
    h, widths = RAGGED_REC
    lines = [rs.randn(h, w, 3).astype(np.float32) for w in widths]
    net = pkg.Net("rec")
    for keep_all in (0, 1, 2):
        out["rec-ragged-keep%d" % keep_all] = _net_case(pkg, net, lambda: net.forward_ragged(lines, keep_all=keep_all))
    net.close()
    imgs = [rs.randn(h, w, 3).astype(np.float32) for h, w in RAGGED_DET]
    net = pkg.Net("det")
    for keep_all in (0, 2):
        out["det-ragged-keep%d" % keep_all] = _net_case(pkg, net, lambda: net.forward_ragged_images(imgs, keep_all=keep_all))
    net.close()
    return out


def pipe_case(pkg):
    """the stages set what a bare Net never has: the fused softmax head's sinks and the detector's bitmap sink"""
    import numpy as np
    card = np.load(os.path.join(ROOT, "tests", "golden", "card_jd_bgr.npy"))
    pipe = pkg.Pipe()
    pipe.timing(True)
    pipe.run([card])
    rows = _rows(pipe.timing_report())
    pipe.close()
    return {"pipe-card": {"launches": rows, "exists": ""}}


def collect(group):
    pkg = _pkg()
    if group == "switch":
        return uniform_cases(pkg, kinds=("det", "rec"))
    out = uniform_cases(pkg)
    out.update(ragged_cases(pkg))
    out.update(pipe_case(pkg))
    return out


def start_switch_children():
    """one child process per switch set, side by side"""
    import subprocess
    return {name: subprocess.Popen([sys.executable, os.path.abspath(__file__), "--group", "switch"], env=dict(os.environ, **env),
                                   stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for name, env in SWITCHES.items()}


def join_switch_children(procs):
    import subprocess
    out = {}
    for name, pr in procs.items():
        try:
            so, se = pr.communicate(timeout=CHILD_TIMEOUT_S)
        except subprocess.TimeoutExpired:
            for q in procs.values():
                q.kill()
            raise RuntimeError("net_launch_list child %s did not finish in %d s" % (name, CHILD_TIMEOUT_S))
        if pr.returncode != 0:
            raise RuntimeError("net_launch_list child %s failed:\n%s" % (name, se[-2000:]))
        out[name] = json.loads(so.splitlines()[-1])
    return out


def collect_all():
    procs = start_switch_children()
    cases = collect("main")
    return {"cases": cases, "switches": join_switch_children(procs)}


if __name__ == "__main__":
    group = sys.argv[sys.argv.index("--group") + 1] if "--group" in sys.argv else None
    res = collect(group) if group else collect_all()
    if not group:
        res = dict({"about": "tools/net_launch_list.py; rows are [launch name, count, flops, bytes]; a case the binder refuses is "
                             "recorded as its error text",
                    "switch_sets": SWITCHES}, **res)
    text = json.dumps(res, separators=(",", ":"), sort_keys=True)
    if not group:  # one case per line
        text = text.replace('},"', '},\n"')
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write(text + "\n")
    else:
        print(text)
