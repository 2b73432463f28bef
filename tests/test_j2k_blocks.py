"""JPEG 2000 requests, the seam between tier-2 and tier-1 (host/j2k_decode.h: parse_coded, tier1, coded_fault) through
host/j2k_check --coded / --tier1.  The yardstick is j2k::parse itself (--frame), which tests/test_j2k_decode.py pins to OpenJPEG:
every comparison is exact equality of integers."""
import glob
import io
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import j2k_blocks as jb  # noqa: E402
import j2k_frames as jf  # noqa: E402

GOLDEN = os.path.join(jf.ROOT, "tests", "golden", "jp2")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return jf.build_check(tmp_path_factory.mktemp("j2kblocks"))


@pytest.fixture(scope="module")
def san(tmp_path_factory):
    return jf.build_check(tmp_path_factory.mktemp("j2kblocks_san"), "-fsanitize=address,undefined", "-fno-sanitize-recover=all")


def golden_files():
    return sorted(glob.glob(os.path.join(GOLDEN, "*.jp2")) + glob.glob(os.path.join(GOLDEN, "*.j2k")))


def both_routes(exe, d, path):
    """(--frame, --coded then --tier1) of one file: per route the frame, or the refusal's text"""
    out = []
    for route in ("frame", "split"):
        dump = os.path.join(str(d), route + ".bin")
        if route == "frame":
            r = subprocess.run([exe, "--frame", path, dump], capture_output=True, text=True)
        else:
            coded = os.path.join(str(d), "coded.bin")
            r = subprocess.run([exe, "--coded", path, coded], capture_output=True, text=True)
            if r.returncode == 0:
                r = subprocess.run([exe, "--tier1", coded, dump], capture_output=True, text=True)
        assert r.returncode in (0, 1), (route, path, r.returncode, r.stderr[-2000:])
        out.append(jf.read_frames(dump)[0] if r.returncode == 0 else r.stderr.strip())
    return out


def same(a, b, name):
    if isinstance(a, str) or isinstance(b, str):
        assert a == b, name
        return
    assert set(a) == set(b), name
    for key in a:
        if key in ("tcs", "steps", "coeffs"):
            assert a[key].dtype == b[key].dtype and np.array_equal(a[key], b[key]), (name, key)
        else:
            assert a[key] == b[key], (name, key)


def test_split_route_equals_parse_over_the_golden_files(exe, tmp_path):
    """every file of tests/golden/jp2: --coded then --tier1 gives the tcs, steps, coeffs and every informative field of --frame;
    no listed block is one decode_tile skips, and passes obeys the descriptor rule"""
    files = golden_files()
    assert len(files) >= 20
    for path in files:
        a, b = both_routes(exe, tmp_path, path)
        assert not isinstance(a, str), (path, a)
        same(a, b, path)
        cd = jb.read_coded(tmp_path / "coded.bin")[0]
        k = cd["cblks"]
        assert cd["ncoeffs"] == len(a["coeffs"]) and len(k) > 0
        assert (k["passes"] >= 1).all() and (k["numbps"] >= 1).all() and (k["passes"] <= 3 * k["numbps"].astype(int) - 2).all()
        assert int((k["byte_off"] + k["byte_len"]).max()) <= len(cd["bytes"])


def variants():
    """(name, Pillow's options): the five progressions, 1 .. 3 layers, the four extreme code-block sizes, tiles, both transforms"""
    out = []
    sizes = [(4, 4), (64, 64), (1024, 4), (4, 1024)]
    k = 0
    for prog in ("LRCP", "RLCP", "RPCL", "PCRL", "CPRL"):
        for layers in (1, 2, 3):
            for irr in (False, True):
                kw = dict(progression=prog, irreversible=irr, codeblock_size=sizes[k % 4])
                if layers > 1:
                    kw.update(quality_layers=[40, 10, 2][:layers], quality_mode="rates")
                if k % 3 == 1:
                    kw.update(tile_size=(48, 40))
                if k % 5 == 2:
                    kw.update(num_resolutions=3)
                out.append(("%s layers %d %s cb %dx%d%s" % (prog, layers, "9/7" if irr else "5/3", *sizes[k % 4], " tiles" if k % 3 == 1 else ""), kw))
                k += 1
    return out


def test_split_route_equals_parse_over_files_written_here(exe, tmp_path):
    """a few dozen files written by Pillow's OpenJPEG over the variants: the split route equals --frame"""
    Image = pytest.importorskip("PIL.Image")
    from PIL import features
    if not features.check_codec("jpg_2000"):
        pytest.skip("Pillow without OpenJPEG")
    rs = np.random.RandomState(11)
    plan = variants()
    assert len(plan) >= 30
    assert {kw["codeblock_size"] for _, kw in plan} == {(4, 4), (64, 64), (1024, 4), (4, 1024)}
    for i, (name, kw) in enumerate(plan):
        w, h = (1100, 70) if kw["codeblock_size"][0] == 1024 else (70, 1100) if kw["codeblock_size"][1] == 1024 else (97, 83)
        smooth = np.add.outer(np.arange(h) * 3, np.arange(w) * 5)[:, :, None] + np.array([0, 80, 160])
        arr = ((smooth + rs.randint(-20, 21, (h, w, 3))) % 256).astype(np.uint8)
        if i % 4 == 3:
            arr = arr[:, :, 0].copy()
        buf = io.BytesIO()
        Image.fromarray(arr).save(buf, "JPEG2000", no_jp2=bool(i % 2), **kw)
        path = tmp_path / ("v%02d.jp2" % i)
        path.write_bytes(buf.getvalue())
        a, b = both_routes(exe, tmp_path, str(path))
        assert not isinstance(a, str), (name, a)
        assert a["layers"] == len(kw.get("quality_layers", [0])) and (a["cbw"], a["cbh"]) == kw["codeblock_size"], name
        same(a, b, name)


def rules():
    """every rule of j2k::coded_fault: (change to a sound descriptor's block record or pool, part of the message)"""
    def blk(i, key, value):
        def f(cd):
            cd["cblks"][i][key] = value
        return f

    def size(i, w, h):
        def f(cd):
            cd["cblks"][i]["w"], cd["cblks"][i]["h"] = w, h
        return f
    return [(blk(0, "w", 0), "1 .. 1024"), (blk(1, "h", 0), "1 .. 1024"), (blk(2, "w", 1025), "1 .. 1024"), (blk(2, "h", 1025), "1 .. 1024"), (size(3, 128, 64), "4096 samples"),
            (blk(4, "orient", 4), "orientation"), (blk(5, "numbps", 0), "bit planes"), (blk(5, "numbps", 31), "bit planes"), (blk(6, "passes", 0), "passes"),
            (blk(6, "passes", 14), "passes"), (blk(7, "tc", 6), "tile-component lies beyond"), (blk(1, "h", 7), "rectangle leaves"), (blk(1, "w", 4), "rectangle leaves"),
            (blk(8, "at", 1 << 20), "rectangle leaves"), (blk(9, "byte_off", 1 << 40), "bytes lie beyond"), (blk(17, "byte_len", 41), "bytes lie beyond"),
            (lambda cd: cd.__setitem__("bytes", cd["bytes"][:-1]), "bytes lie beyond")]


def test_every_descriptor_rule_trips_with_its_message(exe, tmp_path):
    """each rule of j2k::coded_fault refuses (j2k_check --tier1: exit status 1, nothing written, the rule's message); the sound
    descriptor passes, and two overlapping blocks are no fault"""
    rs = np.random.RandomState(2)
    sound = jb.small_coded(rs)
    assert len(sound["cblks"]) == 18
    frames = jb.host_tier1(exe, tmp_path, [sound])
    assert len(frames) == 1 and np.count_nonzero(frames[0]["coeffs"]) > 0
    for n, (change, text) in enumerate(rules()):
        cd = dict(sound, cblks=sound["cblks"].copy(), bytes=sound["bytes"].copy())
        change(cd)
        src, out = tmp_path / ("rule%02d.bin" % n), tmp_path / ("rule%02d.out" % n)
        jb.write_coded(src, [cd])
        r = subprocess.run([exe, "--tier1", str(src), str(out)], capture_output=True, text=True)
        assert r.returncode == 1 and text in r.stderr, (n, text, r.returncode, r.stderr[-500:])
        assert os.path.getsize(out) == 0, n
    cd = dict(sound, cblks=sound["cblks"].copy())
    cd["cblks"][2]["at"] = cd["cblks"][0]["at"]
    cd["cblks"][2]["tc"] = cd["cblks"][0]["tc"]
    assert len(jb.host_tier1(exe, tmp_path, [cd], "overlap")) == 1


def cuts(data, n=24):
    """a spread of byte positions: the first and last few, and evenly spaced ones between"""
    at = sorted(set(list(range(0, 6)) + [len(data) * k // n for k in range(1, n)] + list(range(len(data) - 5, len(data)))))
    return [a for a in at if 0 <= a < len(data)]


def test_truncated_files_give_the_same_result_or_refusal_through_both_routes(exe, tmp_path):
    """three golden files cut at a spread of positions: the split route gives what parse gives - the same frame or the same
    refusal with the same reason"""
    names = [os.path.basename(p) for p in golden_files()]
    # (a JP2 cut short is refused at its boxes; a bare codestream cut in a tile's body decodes what arrived)
    pick = [n for n in names if not n.startswith("card") and n.endswith(".jp2")][:1] + [n for n in names if not n.startswith("card") and n.endswith(".j2k")]
    assert len(pick) == 3
    ok = bad = 0
    for name in pick:
        data = open(os.path.join(GOLDEN, name), "rb").read()
        for at in cuts(data):
            path = tmp_path / "cut.jp2"
            path.write_bytes(data[:at])
            a, b = both_routes(exe, tmp_path, str(path))
            same(a, b, (name, at))
            ok, bad = ok + (not isinstance(a, str)), bad + isinstance(a, str)
    assert ok > 0 and bad > 0


def test_sanitizer_build_runs_the_split_route_clean(san, tmp_path):
    """j2k_check with -fsanitize=address,undefined: --coded and --tier1 over every golden file and over truncated ones exit with
    0 or 1 (a refusal), never with the sanitizer's report"""
    for path in golden_files():
        coded = tmp_path / "g.coded"
        r = subprocess.run([san, "--coded", path, str(coded)], capture_output=True, text=True)
        assert r.returncode == 0, (path, r.stderr[-2000:])
        r = subprocess.run([san, "--tier1", str(coded), str(tmp_path / "g.frames")], capture_output=True, text=True)
        assert r.returncode == 0, (path, r.stderr[-2000:])
    small = [p for p in golden_files() if not os.path.basename(p).startswith("card")]
    for path in small[::4]:
        data = open(path, "rb").read()
        for at in cuts(data, 12):
            cut, coded = tmp_path / "cut.jp2", tmp_path / "cut.coded"
            cut.write_bytes(data[:at])
            r = subprocess.run([san, "--coded", str(cut), str(coded)], capture_output=True, text=True)
            assert r.returncode in (0, 1) and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (path, at, r.stderr[-2000:])
            if r.returncode == 0:
                r = subprocess.run([san, "--tier1", str(coded), str(tmp_path / "cut.frames")], capture_output=True, text=True)
                assert r.returncode == 0 and "runtime error" not in r.stderr, (path, at, r.stderr[-2000:])
    # a broken block list through the sanitizer build: refused, nothing read beyond the pool
    rs = np.random.RandomState(4)
    cd = jb.small_coded(rs)
    cd["cblks"][3]["byte_len"] = 1 << 20
    jb.write_coded(tmp_path / "bad.coded", [cd])
    r = subprocess.run([san, "--tier1", str(tmp_path / "bad.coded"), str(tmp_path / "bad.frames")], capture_output=True, text=True)
    assert r.returncode == 1 and "bytes lie beyond" in r.stderr, r.stderr[-1000:]
