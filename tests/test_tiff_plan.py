"""The plan of a coded TIFF batch (csrc/tiff_plan.h), on the CPU: where each frame's expanded chunks and coded bytes lie, the
chunk records in the order of the launch, the image descriptors of the pixel stage and the Deflate verdict.  The header runs
in host/tiff_plan_check.cpp, a plain host program, built twice: as it is and with -fsanitize=address,undefined; every case
goes through both and nothing of either is loaded into Python.

The printed plan is held to the rules restated here: every frame padded to 256 bytes in the expanded chunks, the pools back to
back; the upload is the records padded to 256, then the pool padded to 256; the records are in the order of the batch, stably
sorted with the longest stream first - on the coded route the LZW chunks so, then the others so; a record reads its chunk's
bytes at the frame's place in the pool and writes the chunk's place in the frame; the descriptors are ordered by sample width
(below 8, 8, 16 bits) with the units of a width numbered through its frames; a Deflate batch reports the first chunk, in the
order of the batch, whose stream gave other than its rows need.  No chunk byte is looked at, so none is made."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "cpp-paddle-ocr_amd", "host")
CODED, DEFLATE, FAX = 0, 1, 2
RECORD_BYTES = {CODED: 32, DEFLATE: 32, FAX: 40}  # TiffChunkDesc, InflateDesc (28 bytes, aligned to 8), TiffFaxDesc
SHORT = "deflate: a chunk's stream does not hold the bytes its rows need (frame %d, chunk %d)"


def pad256(n):
    return (n + 255) // 256 * 256


class Frame:
    """lens: the coded bytes of each chunk, plane by plane, row of chunks by row of chunks; slack: pool bytes behind the last"""

    def __init__(self, width, height, lens, compression, bits=8, photometric=1, samples=1, planar=1, predictor=1, tile=None, t4=0, slack=0):
        self.width, self.height, self.bits, self.photometric, self.samples, self.planar, self.predictor = width, height, bits, photometric, samples, planar, predictor
        self.tw, self.th = tile if tile else (width, height)
        self.compression, self.t4 = compression, t4
        self.across, self.down = -(-width // self.tw), -(-height // self.th)
        self.planes = samples if planar == 2 else 1
        self.row_bytes = (self.tw * (1 if planar == 2 else samples) * bits + 7) // 8
        self.chunk_bytes = self.row_bytes * self.th
        self.total = self.chunk_bytes * self.across * self.down * self.planes
        strips = self.tw == width
        self.chunks, at = [], 0  # (byte_off, byte_len, rows)
        for k, n in enumerate(lens):
            cy = (k // self.across) % self.down
            self.chunks.append((at, n, min(self.th, height - cy * self.th) if strips else self.th))
            at += n
        assert len(self.chunks) == self.across * self.down * self.planes
        self.bytes_len = at + slack

    def text(self):
        head = [self.width, self.height, self.photometric, self.bits, self.samples, self.planar, self.predictor, self.tw, self.th, self.compression, self.t4,
                self.bytes_len, len(self.chunks)]
        return " ".join(map(str, head + [v for c in self.chunks for v in c]))


class Batch:
    """verdicts (Deflate): [(ids or None, produced per chunk in the order of the batch)]"""

    def __init__(self, route, frames, verdicts=()):
        self.route, self.frames, self.verdicts = route, list(frames), list(verdicts)

    def text(self):
        t = ["batch %d %d" % (self.route, len(self.frames))] + [f.text() for f in self.frames]
        if self.route == DEFLATE:
            t.append(str(len(self.verdicts)))
            for ids, produced in self.verdicts:
                t.append(" ".join(map(str, [int(ids is not None)] + list(ids or []) + list(produced))))
        return "\n".join(t)


class Bound:
    def __init__(self, nchunks):
        self.nchunks = nchunks

    def text(self):
        return "bound %d" % self.nchunks


def _grey(w, h, lens, compression, **kw):
    return Frame(w, h, lens, compression, **kw)


# two Deflate frames whose streams grow through the batch: the launch order is the batch order reversed.  need: 40, 40, 30, 30
_DEFLATE = [_grey(10, 8, [5, 10], 8, tile=(10, 4)), _grey(10, 6, [20, 40], 32946, tile=(10, 3))]
CASES = {
    "empty_coded": Batch(CODED, []), "empty_deflate": Batch(DEFLATE, [], [(None, [])]), "empty_fax": Batch(FAX, []),
    "one_coded": Batch(CODED, [_grey(5, 3, [7], 5)]),
    "one_deflate": Batch(DEFLATE, [_grey(5, 3, [7], 8)], [(None, [15]), (None, [14]), ([3], [0])]),
    "one_fax": Batch(FAX, [_grey(9, 3, [7], 4, bits=1)]),
    # expanded chunks of 256, 255 and 257 bytes next to each other, and pools of the same three sizes
    "edges_256": Batch(CODED, [_grey(16, 16, [256], 1), _grey(15, 17, [200], 32773, slack=55), _grey(257, 1, [257], 5), _grey(3, 3, [9], 1)]),
    "edges_256_deflate": Batch(DEFLATE, [_grey(15, 17, [255], 8), _grey(257, 1, [200], 8, slack=57), _grey(16, 16, [256], 8)]),
    # compressions 1, 5 and 32773 across frames, equal lengths inside and across frames: two groups, each stable
    "mixed": Batch(CODED, [_grey(8, 6, [12, 30, 12], 32773, tile=(8, 2)), _grey(8, 4, [30, 12], 5, tile=(8, 2)), _grey(6, 4, [12, 12], 1, tile=(6, 2)),
                           _grey(8, 6, [12, 40, 30], 5, tile=(8, 2)), _grey(4, 2, [30], 32773)]),
    "no_lzw": Batch(CODED, [_grey(8, 4, [9, 9], 1, tile=(8, 2)), _grey(8, 4, [9, 20], 32773, tile=(8, 2))]),
    "only_lzw": Batch(CODED, [_grey(8, 4, [9, 9], 5, tile=(8, 2)), _grey(8, 4, [20, 9], 5, tile=(8, 2))]),
    # 3 x 3 tiles of 16 x 16 over 40 x 40; strips of 3 rows over 7: the last holds one row, need < nominal
    "tiles": Batch(CODED, [_grey(40, 40, [20 + k for k in range(9)], 5, tile=(16, 16)), _grey(11, 7, [8, 8, 3], 32773, tile=(11, 3))]),
    "tiles_deflate": Batch(DEFLATE, [_grey(40, 40, [29 - k for k in range(9)], 8, tile=(16, 16)), _grey(11, 7, [8, 8, 3], 8, tile=(11, 3))]),
    # planar 2: a plane of chunks per sample
    "planes": Batch(CODED, [Frame(6, 5, [10, 4, 11, 5, 12, 6], 5, photometric=2, samples=3, planar=2, tile=(6, 3)), _grey(6, 5, [30], 1)]),
    # 1, 8 and 16 bits interleaved: three kinds of descriptors, the units of each numbered through its frames
    "widths": Batch(CODED, [_grey(9, 5, [45], 1), _grey(70, 5, [9], 5, bits=1), _grey(9, 5, [90], 1, bits=16), _grey(300, 40, [50, 60], 32773, bits=1, tile=(300, 20)),
                            _grey(20, 70, [33], 5), Frame(4, 4, [8], 1, bits=4, photometric=3), Frame(5, 2, [30], 5, photometric=2, samples=3, predictor=2),
                            Frame(5, 2, [40], 1, photometric=5, samples=4), _grey(3, 2, [12], 1, bits=16, photometric=0)]),
    # two widths, T4Options on the Compression 3 frame alone
    "fax": Batch(FAX, [_grey(100, 9, [14, 14, 6], 3, bits=1, tile=(100, 4), t4=5), _grey(33, 4, [14], 4, bits=1, photometric=0), _grey(100, 2, [20], 2, bits=1)]),
    "deflate_short": Batch(DEFLATE, _DEFLATE, [(None, [40, 40, 30, 30]), (None, [40, 39, 0, 30]), (None, [40, 40, 30, 29]), (None, [41, 40, 30, 30])]),
    "deflate_short_ids": Batch(DEFLATE, _DEFLATE, [([9, 4], [40, 39, 0, 30]), ([9, 4], [40, 40, 29, 30])]),
    # the most chunks a launch has workgroups for, and one more
    "bound_at": Bound(0x7fffffff), "bound_above": Bound(0x80000000), "bound_none": Bound(0),
}
BATCHES = [k for k, c in CASES.items() if isinstance(c, Batch)]


@pytest.fixture(scope="module")
def checkers(tmp_path_factory):
    """host/tiff_plan_check.cpp as it is and with AddressSanitizer and UBSan: stand-alone host programs"""
    d = str(tmp_path_factory.mktemp("tiffplan"))
    exes = []
    for name, flags in (("tiff_plan_check", ["-O2"]), ("tiff_plan_check_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exes.append(os.path.join(d, name))
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-o", exes[-1], os.path.join(HOST, "tiff_plan_check.cpp"), "-ldl"])
    return exes


def _ints(line):
    return tuple(map(int, line.split()))


def _parse(out, cases):
    lines = out.splitlines()
    p = 0

    def block(word, width):
        """"<word> <n>" and the n lines after it"""
        nonlocal p
        head = lines[p].split()
        assert head[0] == word and len(head) == 2, lines[p]
        rows = [_ints(l) for l in lines[p + 1:p + 1 + int(head[1])]]
        assert len(rows) == int(head[1]) and all(len(r) == width for r in rows)
        p += 1 + len(rows)
        return rows

    res = []
    for k, c in enumerate(cases):
        assert lines[p] == "case %d" % k
        p += 1
        if isinstance(c, Bound):
            assert lines[p] in ("fits 0", "fits 1")
            res.append(int(lines[p][5:]))
            p += 1
            continue
        r = {"frames": block("frames", 6)}
        assert lines[p].startswith("sizes ")
        r["sizes"] = _ints(lines[p][6:])
        p += 1
        r["records"] = block("records", {CODED: 8, DEFLATE: 7, FAX: 10}[c.route])
        assert lines[p].startswith("kinds ")
        r["kinds"] = _ints(lines[p][6:])
        p += 1
        r["descs"] = block("descs", 22)
        r["short"] = []
        for _ in (c.verdicts if c.route == DEFLATE else ()):
            assert lines[p].startswith("short ")
            n = int(lines[p][6:])
            r["short"].append((n, lines[p + 1] if n >= 0 else None))
            p += 1 + (n >= 0)
        res.append(r)
    assert p == len(lines)
    return res


@pytest.fixture(scope="module")
def plans(checkers):
    """every case through ONE process of each build; both must print the same"""
    text = "\n".join(c.text() for c in CASES.values()) + "\n"
    outs = []
    for exe in checkers:
        r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, (exe, r.returncode, r.stderr[-2000:])
        outs.append(r.stdout)
    assert outs[0] == outs[1]
    return dict(zip(CASES, _parse(outs[0], list(CASES.values()))))


def _layout(c):
    """per frame (off, pool_at, first_chunk), and the batch's expanded bytes, pool and chunks"""
    rows, off, pool, chunks = [], 0, 0, 0
    for f in c.frames:
        rows.append((off, pool, chunks))
        off, pool, chunks = off + pad256(f.total), pool + f.bytes_len, chunks + len(f.chunks)
    return rows, off, pool, chunks


def _launch_order(c):
    """(frame, chunk) in the order of the launch, and the number of LZW records in front (coded route)"""
    batch = [(i, k) for i, f in enumerate(c.frames) for k in range(len(f.chunks))]
    longest_first = lambda group: sorted(group, key=lambda w: -c.frames[w[0]].chunks[w[1]][1])  # stable: ties keep the order of the batch
    if c.route != CODED:
        return longest_first(batch), 0
    lzw = [w for w in batch if c.frames[w[0]].compression == 5]
    return longest_first(lzw) + longest_first([w for w in batch if c.frames[w[0]].compression != 5]), len(lzw)


# ------------------------------------------------------------------------------------------ the tests
@pytest.mark.parametrize("name", BATCHES)
def test_offsets_and_padding(plans, name):
    c, got = CASES[name], plans[name]
    rows, total, pool, chunks = _layout(c)
    assert [g[:3] for g in got["frames"]] == rows
    assert [g[3:] for g in got["frames"]] == [(f.total, f.chunk_bytes, f.row_bytes) for f in c.frames]
    assert all(g[0] % 256 == 0 for g in got["frames"]) and total % 256 == 0
    record_bytes = chunks * RECORD_BYTES[c.route]
    assert got["sizes"][:6] == (total, pool, chunks, record_bytes, pad256(record_bytes), pad256(record_bytes) + pad256(pool))


def test_the_256_byte_edges(plans):
    got = plans["edges_256"]
    assert [g[3] for g in got["frames"]] == [256, 255, 257, 9] and [g[0] for g in got["frames"]] == [0, 256, 512, 1024]
    assert [g[1] for g in got["frames"]] == [0, 256, 511, 768] and got["sizes"][:2] == (1280, 777)           # pools of 256, 255, 257 and 9 bytes
    assert got["sizes"][3:6] == (128, 256, 256 + 1024)
    got = plans["edges_256_deflate"]
    assert [g[0] for g in got["frames"]] == [0, 256, 768] and [g[1] for g in got["frames"]] == [0, 255, 512] and got["sizes"][:2] == (1024, 768)
    assert got["sizes"][3:6] == (96, 256, 256 + 768)                                                           # a pool of exactly three times 256
    for name in ("empty_coded", "empty_deflate", "empty_fax"):
        assert plans[name]["sizes"] == (0,) * 8 and plans[name]["records"] == [] and plans[name]["descs"] == [] and plans[name]["kinds"] == (0,) * 9
    assert plans["one_coded"]["sizes"] == (256, 7, 1, 32, 256, 512, 1, 0) and plans["one_fax"]["sizes"] == (256, 7, 1, 40, 256, 512, 0, 0)


@pytest.mark.parametrize("name", BATCHES)
def test_records_are_in_launch_order_and_say_where_their_chunk_lies(plans, name):
    c, got = CASES[name], plans[name]
    rows, _, _, _ = _layout(c)
    order, lzw = _launch_order(c)
    assert [r[:2] for r in got["records"]] == order                                          # the (frame, chunk) map
    assert got["sizes"][6:] == ((lzw, len(order) - lzw) if c.route == CODED else (0, 0))
    for (i, k), r in zip(order, got["records"]):
        f = c.frames[i]
        byte_off, byte_len, nrows = f.chunks[k]
        assert r[2:5] == (rows[i][1] + byte_off, rows[i][0] + k * f.chunk_bytes, byte_len)  # src, dst, byte_len
        if c.route == FAX:
            assert r[5:] == (nrows, f.chunk_bytes, f.tw, f.compression, f.t4)
        else:
            assert r[5:7] == (nrows * f.row_bytes, f.chunk_bytes) and r[5] <= r[6]          # need, nominal
            assert c.route == DEFLATE or r[7] == f.compression
    if c.route == CODED:
        assert all(r[7] == 5 for r in got["records"][:lzw]) and all(r[7] != 5 for r in got["records"][lzw:])
    for group in (got["records"][:lzw], got["records"][lzw:]):
        assert all(a[4] >= b[4] for a, b in zip(group, group[1:]))                          # the long streams first


def test_record_order_of_the_named_cases(plans):
    # mixed: the LZW frames are 1 and 3 - 40 | 30 30 | 12 12, ties in the order of the batch; then 30 30 | 12 ... of frames 0, 2, 4
    assert [r[:2] for r in plans["mixed"]["records"]] == [(3, 1), (1, 0), (3, 2), (1, 1), (3, 0), (0, 1), (4, 0), (0, 0), (0, 2), (2, 0), (2, 1)]
    assert plans["mixed"]["sizes"][6:] == (5, 6)
    assert plans["no_lzw"]["sizes"][6:] == (0, 4) and [r[:2] for r in plans["no_lzw"]["records"]] == [(1, 1), (0, 0), (0, 1), (1, 0)]
    assert plans["only_lzw"]["sizes"][6:] == (4, 0) and [r[:2] for r in plans["only_lzw"]["records"]] == [(1, 0), (0, 0), (0, 1), (1, 1)]
    # the last strip of 7 rows in strips of 3 holds one: 11 bytes are needed of the 33 written
    assert [r[5:7] for r in plans["tiles"]["records"] if r[0] == 1] == [(33, 33), (33, 33), (11, 33)]
    assert [r[3] for r in sorted(plans["tiles"]["records"]) if r[0] == 0] == [256 * k for k in range(9)]   # 3 x 3 tiles of 16 x 16 bytes
    assert [r[:2] for r in plans["tiles_deflate"]["records"]][:9] == [(0, k) for k in range(9)]
    # three planes of two strips: chunk k of the frame lies at k chunk sizes, whatever its plane
    assert sorted(r[3] for r in plans["planes"]["records"] if r[0] == 0) == [18 * k for k in range(6)]
    assert [r[5:] for r in plans["fax"]["records"]] == [(2, 26, 100, 2, 0), (4, 52, 100, 3, 5), (4, 52, 100, 3, 5), (4, 20, 33, 4, 0), (1, 52, 100, 3, 5)]
    assert [r[:2] for r in plans["deflate_short"]["records"]] == [(1, 1), (1, 0), (0, 1), (0, 0)]           # the batch order reversed


def _lanes(width):
    lanes = 1
    while lanes < 64 and lanes < -(-width // 4):
        lanes *= 2
    return lanes


@pytest.mark.parametrize("name", BATCHES)
def test_image_descriptors(plans, name):
    c, got = CASES[name], plans[name]
    rows, _, _, _ = _layout(c)
    kind = lambda f: 0 if f.bits < 8 else 1 if f.bits == 8 else 2
    count = [sum(1 for f in c.frames if kind(f) == k) for k in range(3)]
    first = [0, count[0], count[0] + count[1]]
    units, want = [0, 0, 0], [[], [], []]
    for i, f in enumerate(c.frames):
        k = kind(f)
        lanes = _lanes(min(f.tw, f.width))
        per_chunk = -(-min(f.th, f.height) // (64 // lanes))
        colour = {2: 3, 5: 4}.get(f.photometric, 1)
        mode = {3: 1, 5: 4, 2: 2}.get(f.photometric, 3 if f.planar == 2 else 0)  # GREY, PALETTE, RGB, GREY_PLANES, CMYK
        want[k].append((rows[i][0], units[k], f.chunk_bytes, f.chunk_bytes * f.across * f.down if f.planar == 2 else 0, f.row_bytes, f.width, f.height, f.tw, f.th,
                        f.across, f.down, f.bits, f.samples, colour, mode, f.predictor, 0, int(f.photometric == 0), 0, lanes, 64 // lanes, per_chunk))
        units[k] += f.across * f.down * per_chunk
    assert got["descs"] == want[0] + want[1] + want[2]
    assert got["kinds"] == tuple(v for k in range(3) for v in (first[k], count[k], units[k]))


def test_descriptors_of_the_three_widths(plans):
    got = plans["widths"]
    assert got["kinds"][0::3] == (0, 3, 7) and got["kinds"][1::3] == (3, 4, 2)
    assert [d[11] for d in got["descs"]] == [1, 1, 4, 8, 8, 8, 8, 16, 16]
    # 70 pixels: 32 lanes a row, 2 rows a unit, 5 rows: 3 units; 300 pixels: 64 lanes, 20 rows a chunk: 20 units each of 2 chunks
    assert [(d[1], d[19], d[20], d[21]) for d in got["descs"][:3]] == [(0, 32, 2, 3), (3, 64, 1, 20), (43, 1, 64, 1)]
    assert got["kinds"][2] == 44
    assert [d[14] for d in got["descs"]] == [0, 0, 1, 0, 0, 2, 4, 0, 0] and [d[17] for d in got["descs"]] == [0] * 8 + [1]
    assert [d[3] for d in plans["planes"]["descs"]] == [36, 0] and plans["planes"]["descs"][0][14] == 2     # planar RGB: two strips a plane


@pytest.mark.parametrize("name", [k for k in BATCHES if CASES[k].route == DEFLATE])
def test_deflate_verdict_is_the_first_short_chunk_of_the_batch(plans, name):
    c, got = CASES[name], plans[name]
    order, _ = _launch_order(c)
    need = [nrows * f.row_bytes for f in c.frames for _, _, nrows in f.chunks]
    batch = [(i, k) for i, f in enumerate(c.frames) for k in range(len(f.chunks))]
    assert len(got["short"]) == len(c.verdicts)
    for (ids, produced), (n, text) in zip(c.verdicts, got["short"]):
        short = [w for w, p, q in zip(batch, produced, need) if p != q]
        if not short:
            assert n == -1
            continue
        i, k = short[0]
        assert order[n] == (i, k) and text == SHORT % (ids[i] if ids else i, k)


def test_deflate_verdicts_of_the_named_cases(plans):
    assert plans["deflate_short"]["short"] == [(-1, None), (2, SHORT % (0, 1)), (0, SHORT % (1, 1)), (3, SHORT % (0, 0))]
    assert plans["deflate_short_ids"]["short"] == [(2, SHORT % (9, 1)), (1, SHORT % (4, 0))]
    assert plans["one_deflate"]["short"] == [(-1, None), (0, SHORT % (0, 0)), (0, SHORT % (3, 0))]
    assert plans["empty_deflate"]["short"] == [(-1, None)]


def test_chunk_count_bound(plans):
    assert plans["bound_at"] == 1 and plans["bound_above"] == 0 and plans["bound_none"] == 1
