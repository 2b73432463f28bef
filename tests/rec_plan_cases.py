"""Cases of host/rec_plan_check.cpp (the recognizer's batching plan, csrc/rec_plan.h, as a plain host program): how a case is written
for it and how its answer is read.  Shared by tests/test_rec_plan.py and tests/test_gpu_srv_pipeline.py."""


class Case:
    """mode: OCR_SORT_STD (0), OCR_SORT_STABLE (1), OCR_SORT_MSVC_STRICT (2) of include/ocr_hip.h"""

    def __init__(self, sizes, seg=None, shape=(48, 320), batch_num=16, mode=0, server=False, cap=4096):
        self.sizes = [(int(w), int(h)) for w, h in sizes]
        self.seg = list(seg) if seg is not None else [0, len(self.sizes)]
        self.imgH, self.imgW = shape
        self.batch_num, self.mode, self.server, self.cap = batch_num, mode, server, cap

    def text(self):
        head = [self.imgH, self.imgW, self.batch_num, self.mode, int(self.server), self.cap, len(self.seg) - 1] + self.seg
        return " ".join(map(str, head + [v for wh in self.sizes for v in wh]))


def parse(out, n):
    """what rec_plan_check printed for n cases: per case ("refused", code, message) or ("plan", items, slots)"""
    lines = out.splitlines()
    res, p = [], 0
    for k in range(n):
        assert lines[p] == "case %d" % k
        if lines[p + 1].startswith("refused "):
            _, code, msg = lines[p + 1].split(" ", 2)
            res.append(("refused", int(code), msg))
            p += 2
            continue
        ni = int(lines[p + 1].split()[1])
        assert lines[p + 1] == "items %d" % ni
        items = [tuple(map(int, l.split())) for l in lines[p + 2:p + 2 + ni]]
        p += 2 + ni
        ns = int(lines[p].split()[1])
        assert lines[p] == "slots %d" % ns
        slots = [tuple(map(int, l.split())) for l in lines[p + 1:p + 1 + ns]]
        p += 1 + ns
        assert all(len(i) == 3 for i in items) and all(len(s) == 3 for s in slots)
        res.append(("plan", items, slots))
    assert p == len(lines)
    return res
