"""Lossy WebP requests, host half: host/vp8_decode.h through the stand-alone checker host/vp8_check.cpp (built with
AddressSanitizer and UBSan: a plain host program, nothing of it is loaded into Python).  The golden files of libwebp's encoder
must give their stored WebPDecodeBGR bytes; damaged files are refused or decode as libwebp decodes them; every descriptor rule
refuses before any device call.  Tests that need libwebp skip without it; the golden test never skips."""
import ctypes
import ctypes.util
import glob
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vp8_frames as vf  # noqa: E402

ROOT = vf.ROOT
GOLDEN = os.path.join(ROOT, "tests", "golden", "webp_lossy")


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return vf.build_check(tmp_path_factory.mktemp("vp8check"), "-fsanitize=address,undefined", "-fno-sanitize-recover=all")


@pytest.fixture(scope="module")
def libwebp():
    try:
        from PIL import features
        if not features.check("webp"):
            pytest.skip("no WebP support on this machine")
        L = ctypes.CDLL(ctypes.util.find_library("webp") or "libwebp.so.7")
    except (ImportError, OSError):
        pytest.skip("no libwebp on this machine")
    L.WebPDecodeBGR.restype = ctypes.c_void_p
    L.WebPDecodeBGR.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
    L.WebPFree.argtypes = [ctypes.c_void_p]

    def decode(data):
        w, h = ctypes.c_int(), ctypes.c_int()
        p = L.WebPDecodeBGR(data, len(data), w, h)
        if not p:
            return None
        a = np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ctypes.c_uint8)), (h.value, w.value, 3)).copy()
        L.WebPFree(p)
        return a

    return decode


def golden_files():
    return sorted(glob.glob(os.path.join(GOLDEN, "*.webp")))


def stored(path):
    npy = path[:-5] + ".npy"
    return np.load(npy if os.path.exists(npy) else os.path.join(GOLDEN, "card_q90.npy"))


def test_golden_files_decode_to_libwebps_bytes(checker, tmp_path):
    """every file of tests/golden/webp_lossy: file -> descriptor (vp8_check --frame) -> vp8::pixels (--pixels) gives the stored
    WebPDecodeBGR bytes, and so does --decode; the set holds B_PRED, four segments, skipped macroblocks, an ALPH file, VP8X"""
    files = golden_files()
    assert len(files) >= 24
    bpred = seg4 = skipped = alph = 0
    for path in files:
        want = stored(path)
        dump, out = tmp_path / "f.bin", tmp_path / "o.bin"
        subprocess.check_call([checker, "--frame", path, str(dump)])
        fr, = vf.read_frames(dump)
        got, = vf.host_pixels(checker, tmp_path, [fr])
        assert got.shape == want.shape and np.array_equal(got, want), os.path.basename(path)
        subprocess.check_call([checker, "--decode", path, str(out)], stdout=subprocess.DEVNULL)
        assert np.array_equal(np.fromfile(out, np.uint8).reshape(want.shape), want), os.path.basename(path)
        bpred += bool(fr["mbs"]["is_i4x4"].any())
        seg4 += len(set(fr["mbs"]["segment"].tolist())) == 4
        skipped += bool(fr["mbs"]["skip"].any())
        alph += b"ALPH" in open(path, "rb").read()[:64]
    assert bpred >= 3 and seg4 >= 1 and skipped >= 1 and alph >= 1


HOSTILE = ["text_17x33_q100_m4", "photo_17x33_q50_m6", "flat_130x33_q5_m6"]


def hostile_files():
    return [os.path.join(GOLDEN, n + ".webp") for n in HOSTILE]


def test_every_prefix_is_refused(checker, tmp_path):
    """every strict prefix of three golden files - every length up to the headers, then every 97th byte - is refused, under the
    sanitizers, without a crash"""
    for path in hostile_files():
        data = open(path, "rb").read()
        cuts = list(range(0, 64)) + list(range(64, len(data), 97)) + [len(data) - 1]
        args = []
        for n in cuts:
            p = tmp_path / ("cut%05d.webp" % n)
            p.write_bytes(data[:n])
            args.append(str(p))
        r = subprocess.run([checker, "--why"] + args, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = r.stdout.strip().splitlines()
        assert len(lines) == len(cuts) and all(line.startswith("refused") for line in lines), [c for c, line in zip(cuts, lines) if not line.startswith("refused")]


def test_flipped_bytes_decode_as_libwebp_or_are_refused(checker, libwebp, tmp_path):
    """single bytes flipped inside the partitions of three golden files, through the sanitizer build: no crash, and where both
    libwebp and the host decoder return pixels they are the same pixels"""
    rs = np.random.RandomState(5)
    both = 0
    for path in hostile_files():
        data = bytearray(open(path, "rb").read())
        start = data.index(b"VP8 ") + 8 + 10
        args, wants = [], []
        for k in range(60):
            at = rs.randint(start, len(data))
            bad = bytearray(data)
            bad[at] ^= 1 << rs.randint(8)
            src = tmp_path / ("flip%03d.webp" % k)
            src.write_bytes(bytes(bad))
            args += [str(src), str(tmp_path / ("flip%03d.bin" % k))]
            wants.append(libwebp(bytes(bad)))
        r = subprocess.run([checker, "--try"] + args, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = r.stdout.strip().splitlines()
        assert len(lines) == len(wants)
        for k, (line, want) in enumerate(zip(lines, wants)):
            if line == "refused" or want is None:
                continue
            got = np.fromfile(args[2 * k + 1], np.uint8).reshape(want.shape)
            assert np.array_equal(got, want), (os.path.basename(path), k)
            both += 1
    assert both >= 30


def test_refusals_say_what_the_issue_fixed(checker, tmp_path):
    """animated files and VP8 chunks without a key-frame header keep the reply "lossy or animated WebP is not decoded"; a sound
    header whose data fails later is a bare decode failure"""
    def riff(chunks):
        body = b"WEBP" + b"".join(t + len(d).to_bytes(4, "little") + d + bytes(len(d) & 1) for t, d in chunks)
        return b"RIFF" + len(body).to_bytes(4, "little") + body

    good = open(golden_files()[5], "rb").read()
    payload = good[20:20 + int.from_bytes(good[16:20], "little")]
    inter = bytes([payload[0] | 1]) + payload[1:]
    badsig = payload[:3] + b"\x9d\x01\x2b" + payload[6:]
    cases = {"zero": riff([(b"VP8 ", bytes(30))]), "short": riff([(b"VP8 ", payload[:8])]), "inter": riff([(b"VP8 ", inter)]), "sig": riff([(b"VP8 ", badsig)]),
             "anim": riff([(b"VP8X", bytes([2]) + bytes(3) + bytes([3, 0, 0, 3, 0, 0])), (b"ANIM", bytes(6)), (b"ANMF", bytes(24))]),
             "cut": riff([(b"VP8 ", payload[:len(payload) // 2])])}
    args = []
    for name, data in cases.items():
        p = tmp_path / (name + ".webp")
        p.write_bytes(data)
        args.append(str(p))
    lines = subprocess.run([checker, "--why"] + args, capture_output=True, text=True, check=True).stdout.strip().splitlines()
    for name, line in zip(cases, lines):
        if name == "cut":
            assert line == "refused: decode failure", line
        else:
            assert line.startswith("refused: lossy or animated WebP is not decoded"), (name, line)


def vp8_frame(pkg, **change):
    rs = np.random.RandomState(1)
    fr = vf.random_frame(rs, 20, 17, "mix", "deltas", "dense")
    f = pkg.Vp8Frame(fr["width"], fr["height"], fr["filter_type"], fr["mbs"], fr["coeffs"])
    for key, value in change.items():
        if key in ("width", "height", "filter_type", "mbs_len", "coeffs_len", "mbs"):
            setattr(f.c, key, value)
        else:
            f.mbs[key][-1] = value
    return f


def test_descriptor_rules_are_refused_before_any_device_call(built, pkg):
    """every rule of ocr_vp8_frame drives ocr_vp8_decode to OCR_ERR_ARG with a message that names it - on a machine with or
    without a GPU: the check comes before the runtime is touched, so nothing was launched, and the output buffer (0xA5) is
    as it was"""
    def refused_as(f, what):
        with pytest.raises(pkg.OcrError, match=what) as e:
            f.decode(fill=0xA5)
        assert e.value.code == -1  # OCR_ERR_ARG
        assert (e.value.out == 0xA5).all()

    refused_as(vp8_frame(pkg, width=0), "1 .. 16383")
    refused_as(vp8_frame(pkg, height=-2), "1 .. 16383")
    refused_as(vp8_frame(pkg, width=16384), "1 .. 16383")
    refused_as(vp8_frame(pkg, filter_type=3), "filter type")
    refused_as(vp8_frame(pkg, mbs_len=3), "fewer macroblock records")
    refused_as(vp8_frame(pkg, width=33), "fewer macroblock records")
    refused_as(vp8_frame(pkg, mbs=None), "fewer macroblock records")
    refused_as(vp8_frame(pkg, is_i4x4=2), "is_i4x4")
    refused_as(vp8_frame(pkg, uvmode=4), "chroma mode")
    refused_as(vp8_frame(pkg, is_i4x4=1, present=0, modes=10), "sub-block mode")
    refused_as(vp8_frame(pkg, is_i4x4=0, modes=4), "16x16 mode")
    refused_as(vp8_frame(pkg, level=64), "filter level")
    refused_as(vp8_frame(pkg, ilevel=64), "interior limit")
    refused_as(vp8_frame(pkg, hev=3), "interior limit")
    refused_as(vp8_frame(pkg, inner=2), "interior limit")
    refused_as(vp8_frame(pkg, present=1 << 25), "25 blocks")
    refused_as(vp8_frame(pkg, is_i4x4=1, modes=0, present=1 << 24), "no Y2 block")
    refused_as(vp8_frame(pkg, nz_uv=1 << 16), "16 bits")
    refused_as(vp8_frame(pkg, coeff_off=1 << 30), "beyond the array")
    refused_as(vp8_frame(pkg, coeffs_len=0, present=1), "beyond the array")


def stream_plan(count):
    """(width, height, prediction, filter, coefficient form, container) of the k-th random stream: every size of the grid `count / 63`
    times, the forms going round at different paces"""
    import vp8_writer as vw
    plan = []
    for k in range(count):
        w, h = vf.WIDTHS[k % 9], vf.HEIGHTS[(k // 9) % 7]
        plan.append((w, h, vw.PRED_FORMS[(k + k // 63) % 15], vw.FILTER_FORMS[(k + k // 15) % 6], vw.COEF_FORMS[(k // 2 + k // 63) % 4], "vp8x" if k % 3 == 0 else "bare"))
    return plan


def expected_blocks(vw, desc, m):
    """the 25 dequantised blocks of a macroblock in raster order, int64 (before the wrap to int16)"""
    seg = m["segment"] if desc["segments"] and desc["segments"]["update_map"] else 0
    y1, y2, uv = vw.quantisers(desc, seg)
    out = np.zeros((25, 16), np.int64)
    if desc["skip_prob"] is not None and m["skip"]:
        return out
    for b in range(25):
        dq = y2 if b == 24 else y1 if b < 16 else uv
        if b == 24 and m["is_i4x4"]:
            continue
        for n in range(1 if b < 16 and not m["is_i4x4"] else 0, 16):
            out[b, vw.ZIGZAG[n]] = int(m["levels"][b][n]) * dq[n > 0]
    return out


def test_random_streams_decode_as_libwebp_decodes_them(checker, libwebp, tmp_path):
    """315 key frames of tests/vp8_writer.py over the size grid and every header field libwebp's encoder does not reach: libwebp
    accepts every one (the writer emits legal streams only), vp8::parse + vp8::pixels give libwebp's bytes, the descriptor holds
    the coefficients the writer coded (quantiser tables, zigzag, the int16 wrap), and the set covers what the decoder can meet"""
    import vp8_writer as vw
    rs = np.random.RandomState(11)
    plan = stream_plan(315)
    descs, args, fargs, wants = [], [], [], []
    for k, (w, h, pred, filt, coef, container) in enumerate(plan):
        d = vw.random_description(rs, w, h, pred, filt, coef, parts=k % 4, segments=bool((k // 4) % 2))
        data = vw.write_webp(d, container)
        src = tmp_path / ("s%03d.webp" % k)
        src.write_bytes(data)
        want = libwebp(data)
        assert want is not None, ("libwebp refuses a stream of the writer", k, plan[k])
        descs.append(d)
        wants.append(want)
        args += [str(src), str(tmp_path / ("s%03d.bin" % k))]
        fargs += [str(src), str(tmp_path / ("s%03d.frame" % k))]
    subprocess.run([checker, "--decode"] + args, check=True, stdout=subprocess.DEVNULL)
    subprocess.run([checker, "--frame"] + fargs, check=True)
    seen = dict(i16=set(), uv=set(), bmode_right=set(), y2=set(), wrap=0, filters=set(), parts=set(), updates=set(), segmaps=0)
    for k, (d, want) in enumerate(zip(descs, wants)):
        got = np.fromfile(args[2 * k + 1], np.uint8).reshape(want.shape)
        assert np.array_equal(got, want), (k, plan[k], d["log2_parts"], bool(d["segments"]))
        fr, = vf.read_frames(fargs[2 * k + 1])
        mw, mh = (d["width"] + 15) >> 4, (d["height"] + 15) >> 4
        assert fr["partitions"] == 1 << d["log2_parts"] and len(fr["mbs"]) == mw * mh
        seen["parts"].add(fr["partitions"])
        seen["updates"].update(d["updates"])
        seen["segmaps"] += fr["segments"] == 4
        for i, (m, rec) in enumerate(zip(d["mbs"], fr["mbs"])):
            x, y = i % mw, i // mw
            where = "corner" if (x, y) == (0, 0) else "top" if y == 0 else "left" if x == 0 else "inside"
            assert rec["is_i4x4"] == m["is_i4x4"] and rec["uvmode"] == m["uvmode"]
            assert rec["modes"].tolist()[:len(m["modes"])] == m["modes"]
            seen["uv"].add((int(rec["uvmode"]), where))
            if rec["is_i4x4"]:
                if x == mw - 1 and y > 0:
                    seen["bmode_right"].update(rec["modes"].tolist())
            else:
                seen["i16"].add((int(rec["modes"][0]), where))
            seen["y2"].add(bool(rec["present"] >> 24 & 1) if not rec["is_i4x4"] else "none")
            if fr["filter_type"] and rec["level"]:
                seen["filters"].add((fr["filter_type"], int(rec["inner"])))
            exact = expected_blocks(vw, d, m)
            wrapped = ((exact + 32768) % 65536 - 32768)
            seen["wrap"] += int((np.abs(exact) > 32767).sum())
            at = int(rec["coeff_off"]) * 16
            for b in range(25):
                if rec["present"] >> b & 1:
                    assert np.array_equal(fr["coeffs"][at:at + 16], wrapped[b]), (k, i, b)
                    at += 16
                else:
                    assert not wrapped[b].any(), (k, i, b)
    for where in ("corner", "top", "left"):
        assert {m for m, at in seen["i16"] if at == where} == {0, 1, 2, 3}, where
        assert {m for m, at in seen["uv"] if at == where} == {0, 1, 2, 3}, where
    assert seen["bmode_right"] == set(range(10))
    assert seen["y2"] >= {True, "none"}
    assert seen["wrap"] > 0
    assert seen["filters"] == {(1, 0), (1, 1), (2, 0), (2, 1)}
    assert seen["parts"] == {1, 2, 4, 8} and seen["segmaps"] > 0
    assert len(seen["updates"]) == 4 * 8 * 3 * 11
