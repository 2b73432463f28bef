"""The host layer's JSON writer with the worker's opt-in char_boxes setting (host/paddle_ocr_hip.h, detail::result_json) on
hand-made words - the test binary's "json" mode, which needs no device: off, the reply is byte for byte what the writer
emitted before the setting existed; on, every word gains "chars":[{"box":[[x,y]x4],"confidence":p}, ..]."""
import json
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "cpp-paddle-ocr_amd", "host")

_WORDS = [
    dict(text='A"b\\中', confidence=np.float32(0.987654321), box=[[1, 2], [30, 2], [30, 14], [1, 14]],
         chars=[([[1, 2], [9, 2], [9, 14], [1, 14]], np.float32(0.5)), ([[9, 2], [20, 2], [20, 14], [9, 14]], np.float32(0.999)),
                ([[20, 2], [30, 2], [30, 14], [20, 14]], np.float32(1.0))]),
    dict(text="", confidence=np.float32(0), box=[[100, 200], [300, 200], [300, 240], [100, 240]], chars=[]),
]


def _esc(s):
    return '"' + s.replace("\\", "\\\\").replace('"', '\\"') + '"'


def _box(b):
    return "[" + ",".join("[%d,%d]" % (p[0], p[1]) for p in b) + "]"


def _writer_before(words):
    """the reply as the writer emitted it before char_boxes existed: jsoncpp's alphabetical keys, %.17g numbers, no blanks"""
    o = '{"height":480,"processing_time_ms":%.17g,"request_id":42,"success":true,"width":640,"words":[' % 12.5
    o += ",".join('{"box":%s,"confidence":%.17g,"text":%s}' % (_box(w["box"]), float(w["confidence"]), _esc(w["text"])) for w in words)
    return o + '],"worker_id":3}'


def test_json_writer_char_boxes(built):
    subprocess.check_call(["make", "-s", "-C", HOST])
    out = subprocess.run([os.path.join(HOST, "test_worker"), "json"], capture_output=True, timeout=120)
    assert out.returncode == 0, out.stderr[-1000:]
    lines = out.stdout.decode("utf-8").splitlines()
    off = [l[len("JSONOFF "):] for l in lines if l.startswith("JSONOFF ")][0]
    on = [l[len("JSONON "):] for l in lines if l.startswith("JSONON ")][0]
    err = [l[len("JSONERR "):] for l in lines if l.startswith("JSONERR ")][0]
    assert off == _writer_before(_WORDS)                      # byte-identical with the setting off
    js = json.loads(on)
    assert [k for k in js] == ["height", "processing_time_ms", "request_id", "success", "width", "words", "worker_id"]
    assert len(js["words"]) == len(_WORDS)
    for g, w in zip(js["words"], _WORDS):
        assert list(g) == ["box", "chars", "confidence", "text"]   # alphabetical, like every other object of the reply
        assert g["box"] == w["box"] and g["text"] == w["text"] and np.float32(g["confidence"]) == w["confidence"]
        assert len(g["chars"]) == len(w["chars"])
        for c, (box, p) in zip(g["chars"], w["chars"]):
            assert list(c) == ["box", "confidence"] and c["box"] == box and np.float32(c["confidence"]) == p
    # dropping the "chars" arrays gives the old reply back
    for g in js["words"]:
        del g["chars"]
    assert js == json.loads(off)
    assert "chars" not in err and json.loads(err)["success"] is False
