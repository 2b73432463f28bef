"""A VP8 key-frame writer for the tests: a boolean ENCODER and everything the key-frame header can say, from a description -
what libwebp's encoder (through Pillow) cannot be made to write.  write_frame(desc) gives the VP8 payload, write_webp(desc)
the file (bare or VP8X).  random_description(rs, ...) draws a legal description; every stream this module writes is legal, so
libwebp must accept it.

The constant tables are read from host/vp8_decode.h: writer and decoder share them, so a wrong entry stays consistent between
the two and only libwebp's pixels expose it (tests/test_vp8_decode.py).

A description is a dict:
  width, height, xscale, yscale (the two ignored bits), profile 0 .. 3
  segments: None, or dict(update_map, update_data, absolute, quantizer[4], strength[4], map_probs[3])
  simple, level, sharpness, lf_delta: None or dict(update, ref[4], mode[4]) (entries None: not sent)
  log2_parts 0 .. 3, base_q, dq[5] (y1dc, y2dc, y2ac, uvdc, uvac), updates {(t, b, c, n): prob}, skip_prob (None: no skip flag)
  mbs: per macroblock dict(segment, skip, is_i4x4, modes (16 or [ymode]), uvmode, levels: 25 x 16 quantised values in ZIGZAG
       order - blocks 0 .. 15 luma, 16 .. 19 U, 20 .. 23 V, 24 Y2 (ignored when is_i4x4; luma position 0 ignored when not))"""
import os
import re
import struct

import numpy as np

HOST = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cpp-paddle-ocr_amd", "host")
DC_PRED, TM_PRED, V_PRED, H_PRED = 0, 1, 2, 3
ZIGZAG = [0, 1, 4, 8, 5, 2, 3, 6, 9, 12, 13, 10, 7, 11, 14, 15]
BANDS = [0, 1, 2, 3, 6, 4, 5, 6, 6, 6, 6, 6, 6, 6, 6, 7, 0]
CATS = [[173, 148, 140], [176, 155, 140, 135], [180, 157, 141, 134, 130], [254, 254, 243, 230, 196, 177, 153, 140, 133, 130, 129]]
MAX_LEVEL = 67 + 2047  # category 6 with all extra bits set
BMODE_TREE = [0, 1, -1, 2, -2, 3, 4, 6, -3, 5, -4, -5, -6, 7, -7, 8, -8, -9]


def _tables():
    text = open(os.path.join(HOST, "vp8_decode.h")).read()

    def table(name):
        m = re.search(r"constexpr uint\d+_t %s\[(\d+)\] = \{([^}]*)\}" % name, text)
        a = np.array([int(v) for v in m.group(2).replace("\n", " ").split(",") if v.strip()])
        assert len(a) == int(m.group(1))
        return a

    return (table("kCoeffProba0").reshape(4, 8, 3, 11), table("kCoeffUpdateProba").reshape(4, 8, 3, 11), table("kBModesProba").reshape(10, 10, 9),
            table("kDcTable"), table("kAcTable"))


COEFF_PROBA0, COEFF_UPDATE, BMODES_PROBA, DC_TABLE, AC_TABLE = _tables()


def _bmode_paths():
    paths = {}

    def walk(i, path):
        for bit in (0, 1):
            nxt = BMODE_TREE[2 * i + bit]
            if nxt > 0:
                walk(nxt, path + [(i, bit)])
            else:
                paths[-nxt] = path + [(i, bit)]

    walk(0, [])
    return paths


BMODE_PATHS = _bmode_paths()


class BoolEncoder:
    """the arithmetic coder the boolean decoder undoes: an interval [low, low + range) of 8 active bits; bytes leave at the top,
    a carry runs back into them"""

    def __init__(self):
        self.out, self.low, self.range, self.pending = bytearray(), 0, 255, 0

    def _carry(self):
        i = len(self.out) - 1
        while self.out[i] == 255:
            self.out[i] = 0
            i -= 1
        self.out[i] += 1

    def put(self, bit, prob):
        split = 1 + (((self.range - 1) * prob) >> 8)
        if bit:
            self.low += split
            self.range -= split
        else:
            self.range = split
        while self.range < 128:
            self.range <<= 1
            self.low <<= 1
            self.pending += 1
        while self.pending >= 8:
            self.pending -= 8
            b = self.low >> (8 + self.pending)
            self.low &= (1 << (8 + self.pending)) - 1
            if b > 255:
                self._carry()
            self.out.append(b & 255)

    def bit(self, b):
        self.put(b, 128)

    def literal(self, v, n):
        for k in range(n - 1, -1, -1):
            self.bit((v >> k) & 1)

    def sliteral(self, v, n):
        self.literal(abs(v), n)
        self.bit(1 if v < 0 else 0)

    def optional(self, v, n):
        """a flag, and the signed value behind it when it is not None"""
        self.bit(0 if v is None else 1)
        if v is not None:
            self.sliteral(v, n)

    def finish(self):
        total = 8 + self.pending
        pad = -total % 8
        low, nbytes = self.low << pad, (total + pad) // 8
        if low >> (8 * nbytes):
            self._carry()
            low &= (1 << (8 * nbytes)) - 1
        return bytes(self.out) + low.to_bytes(nbytes, "big") + bytes(2)  # (two bytes on top: the decoder loads ahead)


def quantisers(desc, segment):
    """(y1, y2, uv) x (dc, ac) of a segment, as the decoder derives them"""
    q = desc["base_q"]
    s = desc["segments"]
    if s:  # (without a data update the decoder's values stay 0 and absolute)
        q = s["quantizer"][segment] + (0 if s["absolute"] else q) if s["update_data"] else 0
    d = desc["dq"]
    clip = lambda v, hi: max(0, min(hi, v))  # noqa: E731
    y2ac = max(8, (int(AC_TABLE[clip(q + d[2], 127)]) * 101581) >> 16)
    return ((int(DC_TABLE[clip(q + d[0], 127)]), int(AC_TABLE[clip(q, 127)])), (2 * int(DC_TABLE[clip(q + d[1], 127)]), y2ac),
            (int(DC_TABLE[clip(q + d[3], 117)]), int(AC_TABLE[clip(q + d[4], 127)])))


def _put_large(e, v, p):
    if v <= 4:
        e.put(0, p[3])
        if v == 2:
            e.put(0, p[4])
        else:
            e.put(1, p[4])
            e.put(v - 3, p[5])
        return
    e.put(1, p[3])
    if v <= 10:
        e.put(0, p[6])
        if v <= 6:
            e.put(0, p[7])
            e.put(v - 5, 159)
        else:
            e.put(1, p[7])
            e.put((v - 7) >> 1, 165)
            e.put((v - 7) & 1, 145)
        return
    e.put(1, p[6])
    cat = 0 if v < 19 else 1 if v < 35 else 2 if v < 67 else 3
    e.put(cat >> 1, p[8])
    e.put(cat & 1, p[9 + (cat >> 1)])
    extra = v - 3 - (8 << cat)
    for k, prob in enumerate(CATS[cat]):
        e.put((extra >> (len(CATS[cat]) - 1 - k)) & 1, prob)


def _put_block(e, proba, t, ctx, levels, first):
    """the tokens of a block from position `first` on; the position behind its last token (what the decoder returns)"""
    last = first
    for n in range(first, 16):
        if levels[n]:
            last = n + 1
    n = first
    p = proba[t][BANDS[n]][ctx]
    while n < 16:
        if n >= last:
            e.put(0, p[0])
            return n
        e.put(1, p[0])
        while not levels[n]:
            e.put(0, p[1])
            n += 1
            p = proba[t][BANDS[n]][0]
        e.put(1, p[1])
        v = abs(int(levels[n]))
        if v == 1:
            e.put(0, p[2])
            nxt = 1
        else:
            e.put(1, p[2])
            _put_large(e, v, p)
            nxt = 2
        e.bit(1 if levels[n] < 0 else 0)
        n += 1
        p = proba[t][BANDS[n]][nxt]
    return 16


def write_frame(desc):
    w, h = desc["width"], desc["height"]
    mw, mh = (w + 15) >> 4, (h + 15) >> 4
    e = BoolEncoder()
    e.bit(0)  # colour space
    e.bit(0)  # clamping type
    s = desc["segments"]
    e.bit(1 if s else 0)
    if s:
        e.bit(s["update_map"])
        e.bit(s["update_data"])
        if s["update_data"]:
            e.bit(s["absolute"])
            for v in s["quantizer"]:
                e.optional(v if v else None, 7)
            for v in s["strength"]:
                e.optional(v if v else None, 6)
        if s["update_map"]:
            for p in s["map_probs"]:
                e.bit(0 if p is None else 1)
                if p is not None:
                    e.literal(p, 8)
    e.bit(desc["simple"])
    e.literal(desc["level"], 6)
    e.literal(desc["sharpness"], 3)
    lf = desc["lf_delta"]
    e.bit(1 if lf else 0)
    if lf:
        e.bit(lf["update"])
        if lf["update"]:
            for v in lf["ref"] + lf["mode"]:
                e.optional(v, 6)
    e.literal(desc["log2_parts"], 2)
    e.literal(desc["base_q"], 7)
    for v in desc["dq"]:
        e.optional(v if v else None, 4)
    e.bit(0)  # refresh entropy probabilities: a key frame keeps nothing anyway
    proba = COEFF_PROBA0.copy()
    for t in range(4):
        for b in range(8):
            for c in range(3):
                for n in range(11):
                    new = desc["updates"].get((t, b, c, n))
                    e.put(0 if new is None else 1, int(COEFF_UPDATE[t, b, c, n]))
                    if new is not None:
                        e.literal(new, 8)
                        proba[t, b, c, n] = new
    e.bit(0 if desc["skip_prob"] is None else 1)
    if desc["skip_prob"] is not None:
        e.literal(desc["skip_prob"], 8)
    proba = proba.tolist()
    nparts = 1 << desc["log2_parts"]
    parts = [BoolEncoder() for _ in range(nparts)]
    seg_p = [255 if p is None else p for p in s["map_probs"]] if s and s["update_map"] else None
    intra_t = [0] * (4 * mw)
    top_nz, top_dc = [0] * mw, [0] * mw
    for y in range(mh):
        intra_l = [0] * 4
        tb = parts[y & (nparts - 1)]
        left_nz = left_dc = 0
        for x in range(mw):
            m = desc["mbs"][y * mw + x]
            if seg_p:
                sg = m["segment"]
                e.put(sg >> 1, seg_p[0])
                e.put(sg & 1, seg_p[1 + (sg >> 1)])
            if desc["skip_prob"] is not None:
                e.put(m["skip"], desc["skip_prob"])
            e.put(0 if m["is_i4x4"] else 1, 145)
            t = intra_t[4 * x:4 * x + 4]
            if not m["is_i4x4"]:
                ym = m["modes"][0]
                e.put(1 if ym in (TM_PRED, H_PRED) else 0, 156)
                if ym in (TM_PRED, H_PRED):
                    e.put(1 if ym == TM_PRED else 0, 128)
                else:
                    e.put(1 if ym == V_PRED else 0, 163)
                t = [ym] * 4
                intra_l = [ym] * 4
            else:
                for by in range(4):
                    ymode = intra_l[by]
                    for bx in range(4):
                        prob = BMODES_PROBA[t[bx]][ymode]
                        ymode = m["modes"][4 * by + bx]
                        for node, bit in BMODE_PATHS[ymode]:
                            e.put(bit, int(prob[node]))
                        t[bx] = ymode
                    intra_l[by] = ymode
            intra_t[4 * x:4 * x + 4] = t
            uv = m["uvmode"]
            e.put(0 if uv == DC_PRED else 1, 142)
            if uv != DC_PRED:
                e.put(0 if uv == V_PRED else 1, 114)
                if uv != V_PRED:
                    e.put(1 if uv == TM_PRED else 0, 183)
            # tokens
            if desc["skip_prob"] is not None and m["skip"]:
                left_nz = top_nz[x] = 0
                if not m["is_i4x4"]:
                    left_dc = top_dc[x] = 0
                continue
            lv = m["levels"]
            if not m["is_i4x4"]:
                nz = _put_block(tb, proba, 1, top_dc[x] + left_dc, lv[24], 0)
                top_dc[x] = left_dc = 1 if nz > 0 else 0
                first, typ = 1, 0
            else:
                first, typ = 0, 3
            tnz, lnz = top_nz[x] & 15, left_nz & 15
            blk = 0
            for by in range(4):
                l = lnz & 1
                for bx in range(4):
                    nz = _put_block(tb, proba, typ, l + (tnz & 1), lv[blk], first)
                    blk += 1
                    l = 1 if nz > first else 0
                    tnz = (tnz >> 1) | (l << 7)
                tnz >>= 4
                lnz = (lnz >> 1) | (l << 7)
            out_t, out_l = tnz, lnz >> 4
            for ch in (0, 2):
                tnz, lnz = (top_nz[x] >> (4 + ch)) & 255, (left_nz >> (4 + ch)) & 255
                for by in range(2):
                    l = lnz & 1
                    for bx in range(2):
                        nz = _put_block(tb, proba, 2, l + (tnz & 1), lv[blk], 0)
                        blk += 1
                        l = 1 if nz > 0 else 0
                        tnz = ((tnz >> 1) | (l << 3)) & 255
                    tnz >>= 2
                    lnz = ((lnz >> 1) | (l << 5)) & 255
                out_t |= ((tnz << 4) << ch) & 255
                out_l |= ((lnz & 0xf0) << ch) & 255
            top_nz[x], left_nz = out_t & 255, out_l & 255
    first_part = e.finish()
    bodies = [p.finish() for p in parts]
    tag = (desc["profile"] << 1) | (1 << 4) | (len(first_part) << 5)
    head = struct.pack("<I", tag)[:3] + b"\x9d\x01\x2a" + struct.pack("<HH", w | (desc["xscale"] << 14), h | (desc["yscale"] << 14))
    sizes = b"".join(struct.pack("<I", len(b))[:3] for b in bodies[:-1])
    return head + first_part + sizes + b"".join(bodies)


def chunk(tag, data):
    return tag + struct.pack("<I", len(data)) + data + bytes(len(data) & 1)


def write_webp(desc, container="bare"):
    body = chunk(b"VP8 ", write_frame(desc))
    if container == "vp8x":
        w, h = desc["width"], desc["height"]
        body = chunk(b"VP8X", bytes(4) + struct.pack("<I", w - 1)[:3] + struct.pack("<I", h - 1)[:3]) + body
    return b"RIFF" + struct.pack("<I", 4 + len(body)) + b"WEBP" + body


PRED_FORMS = ["i16_%d" % m for m in range(4)] + ["b_%d" % m for m in range(10)] + ["mix"]
FILTER_FORMS = ["none", "simple", "normal1", "normal63", "sharp7", "deltas"]
COEF_FORMS = ["skipped", "dc", "dense", "extreme"]


def random_description(rs, width, height, pred="mix", filt="deltas", coef="dense", parts=None, segments=None):
    """pred: "i16_<m>" (chroma mode m too), "b_<m>", "mix"; filt: "none", "simple" (level 20), "normal1", "normal63", "sharp7"
    (level 40, sharpness 7), "deltas" (ref and mode deltas, any level and sharpness); coef: "skipped" (the skip flag on, every
    macroblock skipped), "dc", "dense", "extreme" (the largest token at the largest quantiser among others)"""
    mw, mh = (width + 15) >> 4, (height + 15) >> 4
    d = dict(width=width, height=height, xscale=int(rs.randint(4)), yscale=int(rs.randint(4)), profile=int(rs.randint(4)))
    if segments is None:
        segments = rs.rand() < 0.5
    if segments:
        absolute = int(rs.randint(2))
        update_data = int(rs.rand() < 0.8)
        d["segments"] = dict(update_map=int(rs.rand() < 0.8), update_data=update_data, absolute=absolute,
                             quantizer=[int(v) for v in (rs.randint(0, 128, 4) if absolute else rs.randint(-40, 41, 4))],
                             strength=[int(v) for v in (rs.randint(0, 64, 4) if absolute else rs.randint(-20, 21, 4))],
                             map_probs=[None if rs.rand() < 0.3 else int(rs.randint(1, 256)) for _ in range(3)])
    else:
        d["segments"] = None
    d["simple"] = 1 if filt == "simple" else 0
    d["level"] = {"none": 0, "simple": 20, "normal1": 1, "normal63": 63, "sharp7": 40}.get(filt, int(rs.randint(1, 64)))
    d["sharpness"] = 7 if filt == "sharp7" else int(rs.randint(8)) if filt == "deltas" else 0
    if filt == "deltas":
        opt = lambda: None if rs.rand() < 0.3 else int(rs.randint(-30, 31))  # noqa: E731
        d["lf_delta"] = dict(update=int(rs.rand() < 0.9), ref=[opt() for _ in range(4)], mode=[opt() for _ in range(4)])
    else:
        d["lf_delta"] = None
    d["log2_parts"] = int(rs.randint(4)) if parts is None else parts
    d["base_q"] = 127 if coef == "extreme" else int(rs.randint(128))
    d["dq"] = [0] * 5 if coef == "extreme" else [int(v) if rs.rand() < 0.5 else 0 for v in rs.randint(-15, 16, 5)]
    every = [(t, b, c, n) for t in range(4) for b in range(8) for c in range(3) for n in range(11)]
    share = rs.choice([0.0, 0.1, 0.5, 1.0])
    d["updates"] = {k: int(rs.randint(1, 256)) for k in every if rs.rand() < share}
    d["skip_prob"] = int(rs.randint(1, 256)) if coef == "skipped" or rs.rand() < 0.5 else None
    mbs = []
    for i in range(mw * mh):
        m = dict(segment=int(rs.randint(4)), skip=0)
        if pred.startswith("i16_"):
            m.update(is_i4x4=0, modes=[int(pred[4:])], uvmode=int(pred[4:]))
        elif pred.startswith("b_"):
            m.update(is_i4x4=1, modes=[int(pred[2:])] * 16, uvmode=int(rs.randint(4)))
        else:
            i4 = int(rs.randint(2))
            m.update(is_i4x4=i4, modes=[int(v) for v in rs.randint(10, size=16)] if i4 else [int(rs.randint(4))], uvmode=int(rs.randint(4)))
        levels = np.zeros((25, 16), np.int64)
        if coef == "skipped":
            m["skip"] = 1
        elif coef == "dc":
            on = rs.rand(25) < 0.5
            levels[on, 0] = rs.randint(-40, 41, int(on.sum()))
        elif coef == "dense":
            for b in range(25):
                if rs.rand() < 0.6:
                    k = rs.randint(1, 17)
                    levels[b, :k] = rs.choice([0, 0, 1, -1, 2, -3, 4, 5, -6, 7, 9, -10, 11, 18, -19, 34, 35, -66, 67, 100], k)
        else:
            for b in range(25):
                if rs.rand() < 0.5:
                    k = rs.randint(1, 17)
                    levels[b, :k] = rs.choice([0, MAX_LEVEL, -MAX_LEVEL, 1, -1, 1200, -2048, 67, 66], k)
        if m["is_i4x4"]:
            levels[24] = 0
        else:
            levels[:16, 0] = 0
        if d["skip_prob"] is not None and coef != "skipped" and not levels.any() and rs.rand() < 0.7:
            m["skip"] = 1
        m["levels"] = levels
        mbs.append(m)
    d["mbs"] = mbs
    return d
