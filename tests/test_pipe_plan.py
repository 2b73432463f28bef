"""The pipeline's batch plan (csrc/pipe_plan.h), on the CPU: the detector's resize shape, a slot's layout, the split of a batch
over the chains, the detector's chunks and the bounding-rectangle crops.  The header runs in host/pipe_plan_check.cpp, a plain
host program, built twice: as it is and with -fsanitize=address,undefined; every case goes through both and nothing of either
is loaded into Python.

Shapes and crop rectangles are compared exactly with the oracle's (det_resize_shape, crop_rect).  The layout is held to its
rules (stable (rows, cols) order, one size per group, groups on 256-byte boundaries, images back to back, probability offsets
the running sum of the oracle's map sizes), the split to a restatement of the dealing rule written here (size groups to the
lightest part; a group is cut where the part reaches its share of the batch's pixels plus half an image; at least one image
per deal), the chunks to theirs (in order, within the budget beyond one group, greedy)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "cpp-paddle-ocr_amd", "host")
ALL = 1 << 40  # a budget that takes every group


class Batch:
    def __init__(self, sizes, limit_type="max", side=64, budgets=(0, ALL)):
        self.sizes, self.limit_type, self.side, self.budgets = [tuple(s) for s in sizes], limit_type, side, list(budgets)

    def text(self):
        head = ["batch", int(self.limit_type == "min"), self.side, len(self.budgets)] + self.budgets + [len(self.sizes)]
        return " ".join(map(str, head + [v for s in self.sizes for v in s]))


class Crops:
    def __init__(self, rows, cols, boxes):
        self.rows, self.cols, self.boxes = rows, cols, [[tuple(p) for p in b] for b in boxes]

    def text(self):
        return " ".join(map(str, ["crops", self.rows, self.cols, len(self.boxes)] + [v for b in self.boxes for p in b for v in p]))


def _quad(x0, y0, x1, y1):
    return [(x0, y0), (x1, y0), (x1, y1), (x0, y1)]


SIDES = [(40, 30), (64, 20), (30, 64), (64, 64), (100, 50), (50, 100), (65, 65), (63, 200)]  # below, at and above a side of 64
MIXED = [(40, 40), (20, 30), (40, 40), (20, 30), (40, 40), (20, 20), (20, 30)]              # equal sizes between others
# the order matters to test_same_layout: one_size_again follows one_size, reversed follows sorted
CASES = {
    "empty": Batch([]),
    "one": Batch([(37, 53)]),
    "one_size": Batch([(64, 48)] * 5),
    "one_size_again": Batch([(64, 48)] * 5),
    "sorted": Batch([(10, 10), (10, 12), (12, 10), (12, 12)]),
    "reversed": Batch([(12, 12), (12, 10), (10, 12), (10, 10)]),
    "interleaved": Batch(MIXED),
    "pixel": Batch([(1, 1)]),
    "pixel_among_others": Batch([(5, 7), (1, 1), (16, 16), (1, 1)]),
    "aligned_256": Batch([(16, 16), (32, 8), (16, 16)]),       # 768 bytes each: every image on a 256-byte boundary
    "unaligned": Batch([(5, 7), (3, 3), (5, 7), (9, 11)]),      # 105, 27, 297 bytes
    "max_sides": Batch(SIDES, "max", 64), "min_sides": Batch(SIDES, "min", 64),
    "max_960": Batch([(960, 960), (720, 1280), (1080, 1920), (480, 640)], "max", 960, budgets=(0, 960 * 960, 2 * 960 * 960, ALL)),
    "two": Batch([(30, 30), (20, 20)]), "three": Batch([(30, 30), (20, 20), (30, 30)]),
    "four": Batch([(30, 30)] * 2 + [(20, 20)] * 2), "five": Batch(MIXED[:5]),
    "big_group": Batch([(8, 8), (48, 48), (6, 6)] + [(48, 48)] * 8 + [(4, 4)]),  # nine of one size: cut for 2, 3 and 4 chains
    "big_image": Batch([(8, 8)] * 6 + [(200, 200)]),                             # one image heavier than every share
    "chunks": Batch([(32, 32)] * 2 + [(64, 64)] + [(96, 32)] * 3 + [(128, 128)], "max", 960,
                    budgets=(0, 1, 2048, 4096, 6144, 6145, 15360, 31743, 31744, ALL)),
    "crops_inside": Crops(100, 80, [_quad(10, 5, 50, 20), [(10, 12), (40, 8), (42, 30), (12, 33)], _quad(0, 0, 79, 99)]),
    "crops_partly": Crops(100, 80, [_quad(-5, -7, 20, 10), _quad(70, 90, 120, 130), _quad(-3, 40, 90, 45), [(75, -2), (85, 5), (78, 12), (70, 4)]]),
    "crops_outside": Crops(100, 80, [_quad(80, 0, 90, 5), _quad(0, 100, 5, 110), _quad(-9, -9, -1, -1), _quad(-20, 3, -1, 8)]),
    "crops_points": Crops(100, 80, [[(0, 0)] * 4, [(79, 99)] * 4, [(80, 99)] * 4, [(79, 100)] * 4, [(-1, 0)] * 4, [(40, 50)] * 4]),
    "crops_skipped_middle": Crops(100, 80, [_quad(1, 1, 9, 9), _quad(80, 0, 90, 5), _quad(20, 20, 29, 29), _quad(0, -6, 5, -1), _quad(30, 30, 39, 39)]),
    "crops_none": Crops(100, 80, []),
}
BATCHES = [k for k, c in CASES.items() if isinstance(c, Batch)]
CROPS = [k for k, c in CASES.items() if isinstance(c, Crops)]


@pytest.fixture(scope="module")
def checkers(tmp_path_factory):
    """host/pipe_plan_check.cpp as it is and with AddressSanitizer and UBSan: stand-alone host programs"""
    d = str(tmp_path_factory.mktemp("pipeplan"))
    exes = []
    for name, flags in (("pipe_plan_check", ["-O2"]), ("pipe_plan_check_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exes.append(os.path.join(d, name))
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-o", exes[-1], os.path.join(HOST, "pipe_plan_check.cpp")])
    return exes


def _ints(line):
    return tuple(map(int, line.split()))


def _parse(out, cases):
    lines = out.splitlines()
    p = 0

    def block(word, width, extra=0):
        """"<word> [extra fields] <n>" and the n lines after it"""
        nonlocal p
        head = lines[p].split()
        assert head[0] == word and len(head) == 2 + extra, lines[p]
        rows = [l.split() for l in lines[p + 1:p + 1 + int(head[-1])]]
        assert len(rows) == int(head[-1]) and all(len(r) == width for r in rows)
        p += 1 + len(rows)
        return head[1:-1], rows

    res = []
    for k, c in enumerate(cases):
        assert lines[p] == "case %d" % k
        p += 1
        if isinstance(c, Crops):
            rects = [tuple(map(int, r)) for r in block("rects", 5)[1]]
            res.append({"rects": rects, "lines": [tuple(map(int, r)) for r in block("lines", 5)[1]]})
            continue
        r = {"imgs": [tuple(map(int, x[:7])) + (float.fromhex(x[7]), float.fromhex(x[8])) for x in block("imgs", 9)[1]]}
        r["groups"] = [tuple(map(int, x)) for x in block("groups", 6)[1]]
        word = lines[p].split()
        assert word[0] == "bytes" and word[2] == "probs"
        r["bytes"], r["probs"] = int(word[1]), int(word[3])
        word = lines[p + 1].split()
        assert word[0] == "same"
        r["same"] = (int(word[1]), int(word[2]))
        p += 2
        r["chunks"] = {}
        for b in c.budgets:
            (budget,), rows = block("chunks", 2, extra=1)
            assert int(budget) == b
            r["chunks"][b] = [tuple(map(int, x)) for x in rows]
        r["split"] = {}
        for chains in range(1, 5 if c.sizes else 1):
            assert lines[p] == "split %d %d" % (chains, min(chains, len(c.sizes)))
            p += 1
            parts = []
            for _ in range(min(chains, len(c.sizes))):
                word = lines[p].split()
                assert word[0] == "part" and len(word) == 3
                ni, ng = int(word[1]), int(word[2])
                parts.append(([_ints(l) for l in lines[p + 1:p + 1 + ni]], [_ints(l) for l in lines[p + 1 + ni:p + 1 + ni + ng]]))
                assert all(len(x) == 6 for x in parts[-1][0] + parts[-1][1])
                p += 1 + ni + ng
            r["split"][chains] = parts
        res.append(r)
    assert p == len(lines)
    return res


@pytest.fixture(scope="module")
def plans(checkers, tmp_path_factory):
    """every case through ONE process of each build; both must print the same"""
    path = os.path.join(str(tmp_path_factory.mktemp("pipeplan_cases")), "cases.txt")
    with open(path, "w") as f:
        f.write("\n".join(c.text() for c in CASES.values()) + "\n")
    outs = []
    for exe in checkers:
        r = subprocess.run([exe, path], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, (exe, r.returncode, r.stderr[-2000:])
        outs.append(r.stdout)
    assert outs[0] == outs[1]
    return dict(zip(CASES, _parse(outs[0], list(CASES.values()))))


@pytest.fixture(scope="module")
def O(built):
    import oracle
    return oracle


# ------------------------------------------------------------------------------------------ the tests
@pytest.mark.parametrize("name", BATCHES)
def test_resize_shape_equals_the_oracle(plans, O, name):
    c = CASES[name]
    for rows, cols, _, _, _, rh, rw, fh, fw in plans[name]["imgs"]:
        assert (rh, rw, fh, fw) == O.det_resize_shape(rows, cols, c.limit_type, c.side)


@pytest.mark.parametrize("name", BATCHES)
def test_layout_keeps_its_rules(plans, O, name):
    c, got = CASES[name], plans[name]
    imgs, groups = got["imgs"], got["groups"]
    n = len(c.sizes)
    assert sorted(im[2] for im in imgs) == list(range(n))                                    # orig: a permutation
    assert [im[2] for im in imgs] == sorted(range(n), key=lambda i: c.sizes[i])             # the stable (rows, cols) sort
    assert all((im[0], im[1]) == c.sizes[im[2]] for im in imgs)
    at, end, probs = 0, 0, 0
    for k, (rows, cols, first, count, off, prob_off) in enumerate(groups):
        assert first == at and count >= 1 and off % 256 == 0 and off >= end
        assert off - end < 256                                                               # no more padding than the boundary asks
        assert k == 0 or (rows, cols) != groups[k - 1][:2]
        for j in range(count):
            im = imgs[first + j]
            assert im[:2] == (rows, cols) and im[3] == off + j * rows * cols * 3 and im[4] == probs  # back to back: no overlap
            rh, rw, _, _ = O.det_resize_shape(rows, cols, c.limit_type, c.side)
            probs += rh * rw
        assert prob_off == imgs[first][4]
        at += count
        end = off + count * rows * cols * 3
    assert at == n and got["bytes"] == end and got["probs"] == probs


def test_layout_offsets_at_the_256_byte_boundary(plans):
    assert [im[3] for im in plans["aligned_256"]["imgs"]] == [0, 768, 1536]                 # (16, 16) x 2, then (32, 8): no padding
    assert [g[4] for g in plans["unaligned"]["groups"]] == [0, 256, 512]                    # 27 | 2 x 105 | 297 bytes
    assert [im[3] for im in plans["unaligned"]["imgs"]] == [0, 256, 361, 512] and plans["unaligned"]["bytes"] == 809
    assert plans["pixel"]["bytes"] == 3 and plans["empty"]["bytes"] == 0 and plans["empty"]["groups"] == []


def test_same_layout(plans):
    names = BATCHES
    for prev, name in zip([None] + names[:-1], names):
        key = lambda k: [im[:3] for im in plans[k]["imgs"]] if k else []
        assert plans[name]["same"] == (1, int(key(prev) == key(name))), name
    assert plans["one_size_again"]["same"][1] == 1
    assert plans["reversed"]["same"][1] == 0  # the same sizes in the same places, from other images of the batch
    assert [im[:2] for im in plans["reversed"]["imgs"]] == [im[:2] for im in plans["sorted"]["imgs"]]


def deal(groups, K):
    """the dealing rule of ocr_pipe::run_images: per part its layout indices and its (rows, cols, first in the part, count)"""
    load, index, cut = [0] * K, [[] for _ in range(K)], [[] for _ in range(K)]
    share = -(-sum(g[3] * g[0] * g[1] for g in groups) // K)
    for rows, cols, gfirst, count, _, _ in groups:
        px, first = rows * cols, 0
        while first < count:
            p = load.index(min(load))                        # the lightest part, the first of equals
            left, room = count - first, max(share - load[p], 0)
            n = left
            if left * px > room + px // 2:                   # cut where the part reaches its share plus half an image
                n = min(left, max(1, (room + px // 2) // px))
            cut[p].append((rows, cols, len(index[p]), n))
            index[p] += range(gfirst + first, gfirst + first + n)
            load[p] += n * px
            first += n
    return index, cut


@pytest.mark.parametrize("name", [k for k in BATCHES if CASES[k].sizes])
def test_split_equals_the_dealing_rule(plans, name):
    got = plans[name]
    imgs, groups = got["imgs"], got["groups"]
    for chains in range(1, 5):
        parts = got["split"][chains]
        K = min(chains, len(imgs))
        assert len(parts) == K
        assert sorted(x[0] for pi, _ in parts for x in pi) == list(range(len(imgs)))       # every layout index in exactly one part
        index, cut = deal(groups, K)
        for p, (pi, pg) in enumerate(parts):
            assert [x[0] for x in pi] == index[p] and [g[:4] for g in pg] == cut[p]
            assert all(x[1:] == imgs[x[0]][:5] for x in pi)                                 # the layout's own records
            for g in pg:
                assert g[4:] == pi[g[2]][4:]                                                # re-based: off / prob_off of its first image
                assert all(x[1:3] == g[:2] for x in pi[g[2]:g[2] + g[3]])
                assert [x[0] for x in pi[g[2]:g[2] + g[3]]] == list(range(pi[g[2]][0], pi[g[2]][0] + g[3]))  # neighbours in the layout
            assert sum(g[3] for g in pg) == len(pi)  # (a part may stay empty: two 1 x 1 images are one deal)


def test_split_cuts_a_big_group_and_keeps_a_big_image_whole(plans):
    for chains in (2, 3, 4):
        parts = plans["big_group"]["split"][chains]
        assert sum(1 for _, pg in parts for g in pg if g[:2] == (48, 48)) >= chains         # the nine 48 x 48 images: cut for every chain
        px = [sum(x[1] * x[2] for x in pi) for pi, _ in parts]
        assert max(px) - min(px) <= 48 * 48                                                  # within an image of each other
    parts = plans["big_image"]["split"][2]
    assert sorted(len(pi) for pi, _ in parts) == [1, 6]
    assert plans["one_size"]["split"][2][0][1] == [(64, 48, 0, 3, 0, 0)] and len(plans["one_size"]["split"][2][1][0]) == 2


@pytest.mark.parametrize("name", BATCHES)
def test_chunks_are_in_order_within_budget_and_greedy(plans, O, name):
    c, got = CASES[name], plans[name]
    gpx = []
    for rows, cols, _, count, _, _ in got["groups"]:
        rh, rw, _, _ = O.det_resize_shape(rows, cols, c.limit_type, c.side)
        gpx.append(count * rh * rw)
    for budget, chunks in got["chunks"].items():
        at = 0
        for k, (g0, g1) in enumerate(chunks):
            assert g0 == at and g1 > g0
            at = g1
            assert g1 - g0 == 1 or sum(gpx[g0:g1]) <= budget
            if k + 1 < len(chunks):
                assert sum(gpx[g0:g1 + 1]) > budget  # greedy: the next group did not fit
        assert at == len(gpx)
    assert got["chunks"][0] == [(g, g + 1) for g in range(len(gpx))]          # every group its own chunk
    assert got["chunks"][ALL] == ([(0, len(gpx))] if gpx else [])            # everything in one chunk


def test_chunk_boundaries(plans):
    got = plans["chunks"]["chunks"]  # map pixels per group: 2048, 4096, 9216, 16384
    assert [g[3] for g in plans["chunks"]["groups"]] == [2, 1, 3, 1]
    assert got[1] == got[2048] == got[4096] == [(0, 1), (1, 2), (2, 3), (3, 4)]
    assert got[6144] == got[6145] == [(0, 2), (2, 3), (3, 4)]
    assert got[15360] == [(0, 3), (3, 4)] == got[31743] and got[31744] == [(0, 4)]


@pytest.mark.parametrize("name", CROPS)
def test_crop_rectangles_equal_the_oracle(plans, O, name):
    c, got = CASES[name], plans[name]
    want = [O.crop_rect(b, c.rows, c.cols) for b in c.boxes]
    assert len(got["rects"]) == len(want)
    for (ok, *rect), w in zip(got["rects"], want):
        assert bool(ok) == (w is not None) and (w is None or tuple(rect) == w)
    kept = [w for w in want if w is not None]
    # a line's box index is its running index in the image, not its box's (the reference pairs text k with box k)
    assert got["lines"] == [w + (k,) for k, w in enumerate(kept)]


def test_crop_cases_cover_what_they_name(plans):
    assert all(r[0] for r in plans["crops_inside"]["rects"]) and plans["crops_inside"]["rects"][2] == (1, 0, 0, 80, 100)
    assert plans["crops_partly"]["rects"][:2] == [(1, 0, 0, 21, 11), (1, 70, 90, 10, 10)] and all(r[0] for r in plans["crops_partly"]["rects"])
    assert not any(r[0] for r in plans["crops_outside"]["rects"]) and plans["crops_outside"]["lines"] == []
    assert [r[0] for r in plans["crops_points"]["rects"]] == [1, 1, 0, 0, 0, 1]
    assert plans["crops_points"]["rects"][1] == (1, 79, 99, 1, 1)
    assert [r[0] for r in plans["crops_skipped_middle"]["rects"]] == [1, 0, 1, 0, 1]
    assert [l[4] for l in plans["crops_skipped_middle"]["lines"]] == [0, 1, 2]
    assert plans["crops_none"] == {"rects": [], "lines": []}
