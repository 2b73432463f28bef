"""The case table of the server GEMM family's own tests (HIP-free): seeded synthetic plans and parameters, the input shapes, and for
every op WHICH branch of srv_gemm_kernel / srv_conv3_kernel / the fused forms it is there for.  tests/test_srv_gemm_cases.py proves
the table on the CPU (the branches really occur, three references agree on it, every srv_ref.GEMM_MUTATIONS entry separates on it);
tests/test_gpu_srv_gemm.py runs the device on it under every tile configuration.

The plans are this file's own text.  Producers are 1x1 convs from the 3-channel input to each channel count an op under test reads
(what a producer computes does not matter: a test may upload other data into its tensor); every op under test with an f16 output
also gets a follower, a thin linear that reads it, so that a pad channel that is not a clean zero reaches a next product.

Which (configuration, op) pairs the f16 build refuses is PREDICTED here from the rules srv_kernels.h / srv_kernels.hip state in
their comments (never by asking gemm_config_ok):
  * a tile whose f32 epilogue image does not fit LDS (BM (BN + 4) 4 > 160 KB) or whose thread count is no multiple of BN / 8 (192
    columns) has the register epilogues only: no transposed conv, no f32 output (but the CTC partials);
  * the halo form takes f16 3x3 stride-1 pad-1 convs on whole 64-channel tiles without a residual, and nothing else;
  * every other tile takes every op of a keep_all binding."""
import re
import zlib

import numpy as np

REASON_BIG = "a big tile has the register epilogues only"
REASON_HALO = "the halo form takes f16 3x3 stride-1 convs on whole channel tiles"

SHAPES = {
    # M = 1, 63, 65, 255, 256, 257, 513: around every BM (64, 128, 256); images that end inside a pixel tile; a single-column map
    "A": ((1, 1, 1), (1, 3, 21), (1, 5, 13), (3, 5, 17), (2, 8, 16), (1, 257, 1), (3, 9, 19)),
    # below, on and one step past the 16 x 16 halo tile; 24 x 40: every concat depth (H, W multiples of 8) with partial halo tiles
    "B": ((1, 2, 2), (2, 16, 16), (1, 18, 34), (3, 32, 16), (1, 24, 40)),
    # token counts around the fused MLP's 128-token tile
    "C": ((1, 1, 1), (1, 1, 127), (1, 1, 128), (1, 1, 129), (3, 1, 43)),
}
CTC_HEADS = ((448, 13), (64, 64), (192, 200))   # (cin, cout) of the plans "T<cout>": one producer and the f32 output linear
CTC_SHAPES = ((1, 1, 1), (1, 5, 13), (1, 257, 1))
MLP_WIDTHS = (192, 256, 64)                     # 64: no fused instantiation, the pair must stay two launches


def up8(c):
    return (c + 7) // 8 * 8


def _rs(name):
    return np.random.RandomState(zlib.crc32(name.encode()) & 0x7fffffff)


def _param(name, dims):
    """seeded values: weights N(0, 1 / fan_in) (outputs of unit-variance inputs stay O(1): finite in f16), the rest large enough to
    show when it is dropped"""
    rs, suf = _rs(name), name.rsplit(".", 1)[-1]
    if suf == "w":
        fan = dims[0] if len(dims) == 2 or name.startswith("dc") else int(np.prod(dims[1:]))
        v = rs.randn(*dims) / np.sqrt(fan)
    elif suf == "b":
        v = rs.uniform(-0.5, 0.5, dims)
    elif suf == "scale":
        v = rs.uniform(0.7, 1.3, dims)
    elif suf in ("offset", "mean"):
        v = rs.uniform(-0.3, 0.3, dims)
    elif suf == "variance":
        v = rs.uniform(0.5, 1.5, dims)
    elif suf == "g":
        v = rs.uniform(0.9, 1.1, dims)
    else:
        raise ValueError(name)
    return v.astype(np.float32)


class Plan:
    """ops in plan order: dict(label, kind, kv text, o, role "producer" | "support" | "test" | "follower" | "out", branch, of)"""

    def __init__(self, name):
        self.name, self.ops, self.params, self.nt = name, [], {}, 1

    def p(self, name, *dims):
        self.params.setdefault(name, list(dims))
        return name

    def add(self, label, role, kind, text, branch="", of=None, live=True):
        o = self.nt
        self.nt += 1
        self.ops.append(dict(label=label, role=role, kind=kind, text=text, o=o, branch=branch, of=of, live=live))
        return o

    def tid(self, label):
        return next(op["o"] for op in self.ops if op["label"] == label)

    def producer(self, c, live=True):
        return self.add("p%d" % c, "producer", "conv", "i=0 cin=3 cout=%d kh=1 kw=1 sh=1 sw=1 ph=0 pw=0 w=%s" % (c, self.p("p%d.w" % c, c, 3, 1, 1)), live=live)

    def ep(self, label, cout, stages):
        out = []
        for st in stages:
            if st == "bias":
                out.append("bias:" + self.p(label + ".b", cout))
            elif st == "bn":
                out.append("bn:%s,1e-05" % ",".join(self.p("%s_bn.%s" % (label, s), cout) for s in ("scale", "offset", "mean", "variance")))
            else:
                out.append(st)
        return (" ep=" + "|".join(out)) if out else ""

    def tested(self, label, kind, text, cout, branch, follower=True, live=True):
        o = self.add(label, "test", kind, text, branch, live=live)
        if follower:
            self.add(label + ">", "follower", "linear", "i=%d cin=%d cout=8 w=%s" % (o, cout, self.p(label + ">.w", cout, 8)), of=label, live=live)
        return o

    def linear(self, label, i, cin, cout, branch, stages=(), **kw):
        return self.tested(label, "linear", "i=%d cin=%d cout=%d w=%s%s" % (i, cin, cout, self.p(label + ".w", cin, cout), self.ep(label, cout, stages)), cout, branch, **kw)

    def conv(self, label, i, cin, cout, k, s, pd, branch, stages=("bias",), **kw):
        w = self.p(label + ".w", cout, cin, k[0], k[1])
        text = "i=%d cin=%d cout=%d kh=%d kw=%d sh=%d sw=%d ph=%d pw=%d w=%s%s" % (i, cin, cout, k[0], k[1], s[0], s[1], pd[0], pd[1], w, self.ep(label, cout, stages))
        return self.tested(label, "conv", text, cout, branch, **kw)

    def deconv(self, label, i, cin, cout, branch, stages, **kw):
        text = "i=%d cin=%d cout=%d w=%s%s" % (i, cin, cout, self.p("dc" + label + ".w", cin, cout, 2, 2), self.ep(label, cout, stages))
        return self.tested(label, "deconv", text, cout, branch, follower=kw.pop("follower", cout > 1), **kw)

    # ---- text
    def text(self, only=None, with_out=True):
        """the plan; only: labels of the ops under test to keep (their followers go with them; producers and support ops always
        stay).  Without the plan's own `out` op the output is a 1x1 max pool of the first producer (an f16 tensor no GEMM writes)"""
        keep = []
        for op in self.ops:
            if not op["live"]:
                continue
            if op["role"] == "out" and not with_out:
                continue
            if only is not None and ((op["role"] == "test" and op["label"] not in only) or (op["role"] == "follower" and op["of"] not in only)):
                continue
            keep.append(op)
        written = {0}
        for op in list(keep):  # (an op whose input went out with `only` goes too: plan B's map deconv behind the head tail's first)
            reads = [int(t) for m in re.findall(r"\bi=([\d,]+)", op["text"]) for t in m.split(",")] + [int(t) for t in re.findall(r"add(?:t|up):(\d+)", op["text"])]
            if all(t in written for t in reads):
                written.add(op["o"])
            else:
                keep.remove(op)
        lines = ["# synthetic plan of tests/srv_gemm_cases.py - the tests' own text", "plan %s ntensors=%d" % (self.name, self.nt + 1)]
        names = set(re.split(r"[=:,| ]", " ".join(op["text"] for op in keep)))
        lines += ["# param %s %s" % (n, ",".join(str(d) for d in self.params[n])) for n in self.params if n in names]
        lines += ["%s %s o=%d" % (op["kind"], op["text"], op["o"]) for op in keep]
        outs = [op for op in keep if op["role"] == "out"]
        if outs:
            lines.append("output i=%d" % outs[0]["o"])
        else:
            lines.append("pool i=%d kh=1 kw=1 sh=1 sw=1 ph=0 pw=0 type=max o=%d" % (self.ops[0]["o"], self.nt))
            lines.append("output i=%d" % self.nt)
        return "\n".join(lines) + "\n"

    def weights(self, text=None):
        names = self.params if text is None else [ln.split()[2] for ln in text.splitlines() if ln.startswith("# param ")]
        return {n: _param(n, self.params[n]) for n in names}

    def tests(self):
        return [op for op in self.ops if op["role"] in ("test", "out") and op["live"]]


ACTS = ("relu", "gelu", "hswish", "sigmoid")


def plan_a():
    P = Plan("synth_a")
    p = {c: P.producer(c) for c in (64, 128, 192, 448, 24, 96, 32, 72)}
    P.linear("l64_64", p[64], 64, 64, "nkt 1 (f16), x1")
    P.linear("l128_72", p[128], 128, 72, "N no multiple of 64")
    P.linear("l192_200", p[192], 192, 200, "nkt 3")
    P.linear("l448_13", p[448], 448, 13, "nkt 7 > every NS; Ncols no multiple of 8; pad channels", ("bias",))
    P.linear("l24_264", p[24], 24, 264, "K below one tile; x1 off")
    P.linear("l96_576", p[96], 96, 576, "192- and 256-wide column tiles, partial and exact")
    for label, st in (("e_bias", ("bias",)), ("e_bn", ("bn",)), ("e_bias_bn", ("bias", "bn")), ("e_addt", ("bias", "addt:%d" % p[72])),
                      ("e_relu", ("bias", "act:relu")), ("e_gelu", ("bias", "act:gelu")), ("e_hswish", ("bn", "act:hswish")),
                      ("e_sigmoid", ("bias", "addt:%d" % p[72], "act:sigmoid"))):
        P.linear(label, p[128], 128, 72, "epilogue " + "|".join(s.split(":")[0] + (":" + s.split(":")[1] if s.startswith("act") else "") for s in st), st)
    P.conv("c3_3", 0, 3, 40, (3, 3), (1, 1), (1, 1), "cin_shift >= 0 (8 stored channels)")
    P.conv("c3_24", p[24], 24, 40, (3, 3), (1, 1), (1, 1), "cin_shift -2 (division)")
    P.conv("c3_32", p[32], 32, 48, (3, 3), (1, 1), (1, 1), "cin_shift >= 0 (f16: 32 channels)", ("bn", "act:relu"))
    P.conv("c3_64", p[64], 64, 64, (3, 3), (1, 1), (1, 1), "cin_shift -1; K order 1 (f16); halo-eligible", ("bias", "act:relu"))
    P.conv("c3_128", p[128], 128, 72, (3, 3), (1, 1), (1, 1), "cin_shift -1; K order 1 (f16); halo-eligible; partial column tile", ("bn",))
    P.conv("c3_64_s2", p[64], 64, 64, (3, 3), (2, 2), (1, 1), "stride 2")
    P.conv("c1_64_s2", p[64], 64, 72, (1, 1), (2, 2), (0, 0), "strided 1x1")
    P.conv("c1x3_32", p[32], 32, 40, (1, 3), (1, 1), (0, 1), "asymmetric kernel")
    P.conv("c3x1_32", p[32], 32, 40, (3, 1), (2, 1), (1, 0), "asymmetric kernel and stride")
    P.conv("c5_3", 0, 3, 24, (5, 5), (1, 1), (2, 2), "5x5 taps")
    P.deconv("d64_64", p[64], 64, 64, "deconv, 256 GEMM rows", ("bias", "act:relu"))
    P.deconv("d32_24", p[32], 32, 24, "deconv, 96 GEMM rows", ("bias", "bn"))
    P.deconv("d64_1", p[64], 64, 1, "the map kernel", ("bias", "act:sigmoid"))
    P.add("out", "out", "linear", "i=%d cin=128 cout=72 w=%s%s" % (p[128], P.p("out.w", 128, 72), P.ep("out", 72, ("bias",))), "the plan's output linear: f32 out")
    return P


CAT_UPS = ((1,), (2, 1), (4, 2, 1), (8, 4, 2, 1))


def plan_b(shape):
    """even H, W; a concat of depth d needs H and W multiples of its largest factor - the ops of a deeper one are left out (their tensor
    ids stay) at a shape that has none"""
    _, H, W = shape
    assert H % 2 == 0 and W % 2 == 0
    P = Plan("synth_b")
    src = {1: [P.producer(64)] + [P.add("p64_%d" % k, "producer", "conv", "i=0 cin=3 cout=64 kh=1 kw=1 sh=1 sw=1 ph=0 pw=0 w=%s" % P.p("p64_%d.w" % k, 64, 3, 1, 1)) for k in (1, 2, 3)]}
    for f in (2, 4, 8):
        ok = H % f == 0 and W % f == 0
        src[f] = [P.add("q%d_%d" % (f, k), "support", "pool", "i=%d kh=2 kw=2 sh=2 sw=2 ph=0 pw=0 type=max" % src[f // 2][k], live=ok) for k in range(4)]
    q2 = src[2][0]
    P.linear("u_lin", src[1][0], 64, 64, "addup residual, linear", ("bias", "addup:%d,2" % q2))
    P.linear("u_relu", src[1][1], 64, 64, "addup residual behind an activation", ("addup:%d,2" % q2, "act:relu"))
    P.conv("u_c3", src[1][0], 64, 64, (3, 3), (1, 1), (1, 1), "addup residual, 3x3 conv (no halo form)", ("bias", "addup:%d,2" % q2, "act:relu"))
    for d, ups in enumerate(CAT_UPS, 1):
        ok = H % ups[0] == 0 and W % ups[0] == 0
        ins = [src[u][j] for j, u in enumerate(ups)]
        c = P.add("cat%d" % d, "support", "concat", "i=%s up=%s c=%d" % (",".join(map(str, ins)), ",".join(map(str, ups)), 64 * d), live=ok)
        cout = 72 if d == 2 else 64
        P.conv("cat%d_c3" % d, c, 64 * d, cout, (3, 3), (1, 1), (1, 1), "concat of %d sources up=%s folded into the halo form" % (d, ups), ("bias", "act:relu"), follower=False, live=ok)
    P.deconv("ht1", src[1][2], 64, 64, "head tail: deconv 64 -> 64 | relu", ("bias", "act:relu"), follower=False)
    # (ht1's only reader is the map deconv below: the pair fuses in the production binding)
    P.add("out", "out", "deconv", "i=%d cin=64 cout=1 w=%s%s" % (P.tid("ht1"), P.p("dcht2.w", 64, 1, 2, 2), P.ep("ht2", 1, ("bias", "act:sigmoid"))), "head tail: deconv 64 -> 1 | sigmoid")
    return P


def plan_c():
    P = Plan("synth_c")
    for C in MLP_WIDTHS:
        p = P.producer(C)
        l = P.add("ln%d" % C, "support", "ln", "i=%d eps=1e-05 g=%s b=%s" % (p, P.p("ln%d.g" % C, C), P.p("ln%d.b" % C, C)))
        f1 = P.linear("fc1_%d" % C, l, C, 4 * C, "MLP fc1 C = %d" % C, ("bias", "act:gelu"), follower=False)
        P.linear("fc2_%d" % C, f1, 4 * C, C, "MLP fc2 + residual C = %d" % C, ("bias", "addt:%d" % l), follower=False)
    P.add("out", "out", "linear", "i=%d cin=64 cout=16 w=%s%s" % (P.tid("fc2_64"), P.p("out.w", 64, 16), P.ep("out", 16, ("bias",))), "output")
    return P


def plan_t(cin, cout):
    P = Plan("synth_t%d" % cout)
    p = P.producer(cin)
    P.add("out", "out", "linear", "i=%d cin=%d cout=%d w=%s%s" % (p, cin, cout, P.p("out.w", cin, cout), P.ep("out", cout, ("bias",))), "CTC head, %d columns" % cout)
    return P


def plan(name, shape=None):
    if name == "A":
        return plan_a()
    if name == "B":
        return plan_b(shape)
    if name == "C":
        return plan_c()
    return plan_t(*[h for h in CTC_HEADS if "T%d" % h[1] == name][0])


def x_of(name, shape):
    return _rs("x %s %s" % (name, shape)).randn(*shape, 3).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------ geometry
def parse_op(op):
    kv = dict(t.split("=", 1) for t in op["text"].split())
    return kv, {k: int(v) for k, v in kv.items() if re.fullmatch(r"-?\d+", v)}


def geometry(op, in_shape, half):
    """what srv_net.hip's bind derives for a GEMM launch of `op` on an input of (N, H, W): dict(M, K, nkt, ncols, x1, cin_shift,
    korder, OH, OW)"""
    kv, n = parse_op(op)
    N, H, W = in_shape
    BK = 64 if half else 32
    cin_s = up8(n["cin"])
    kh, kw, sh, sw, ph, pw = (n.get(k, d) for k, d in (("kh", 1), ("kw", 1), ("sh", 1), ("sw", 1), ("ph", 0), ("pw", 0)))
    OH, OW = ((H + 2 * ph - kh) // sh + 1, (W + 2 * pw - kw) // sw + 1) if op["kind"] == "conv" else (H, W)
    K = kh * kw * cin_s
    x1 = (kh, kw, sh, sw, ph, pw) == (1, 1, 1, 1, 0, 0) and K % BK == 0
    shift = -1
    if not x1 and cin_s % BK:
        shift = cin_s.bit_length() - 1 if cin_s & (cin_s - 1) == 0 else -2
    return dict(M=N * OH * OW, K=K, nkt=-(-K // BK), ncols=4 * n["cout"] if op["kind"] == "deconv" else n["cout"], x1=int(x1), cin_shift=shift,
                korder=int(half and op["kind"] == "conv" and kh * kw > 1 and cin_s % 64 == 0), OH=OH, OW=OW, k=(kh, kw), s=(sh, sw), p=(ph, pw))


def conv_form(op):
    """the name a conv op's form goes by in the coverage condition "every id that takes convs runs every conv form it accepts" """
    g = geometry(op, (1, 8, 8), True)
    return "k%dx%d s%dx%d shift%d order%d" % (g["k"] + g["s"] + (g["cin_shift"], g["korder"]))


# ------------------------------------------------------------------------------------------------------------ tile table
def tile_of(name):
    """a configuration's name as the library states it -> dict(form "gemm" | "reg" | "halo", BM, BN, NS)"""
    m = re.fullmatch(r"halo16x16x(\d+)", name)
    if m:
        return dict(form="halo", BM=256, BN=int(m.group(1)), NS=3)
    BM, BN, WM, WN, NS = map(int, re.fullmatch(r"(\d+)x(\d+)/(\d+)x(\d+)/s(\d+)", name).groups())
    big = BM * (BN + 4) * 4 > 160 * 1024 or (64 * WM * WN) % (BN // 8) != 0   # GemmGeom::BIG as srv_kernels.hip states it
    return dict(form="reg" if big else "gemm", BM=BM, BN=BN, NS=NS)


def predicted_refusal(tile, op):
    """the reason the f16 build refuses `op` (an op of a keep_all binding that runs as a GEMM launch) on `tile`, None: it runs"""
    kv, n = parse_op(op)
    if op["kind"] == "deconv" and n["cout"] == 1:
        return None                     # (deconv_map_kernel: no GEMM launch)
    if tile["form"] == "reg":
        return REASON_BIG if op["kind"] == "deconv" or op["role"] == "out" else None
    if tile["form"] == "halo":
        ok = (op["kind"] == "conv" and (n["kh"], n["kw"], n["sh"], n["sw"], n["ph"], n["pw"]) == (3, 3, 1, 1, 1, 1) and up8(n["cin"]) % 64 == 0
              and "addt:" not in op["text"] and "addup:" not in op["text"])
        return None if ok else REASON_HALO
    return None


def gemm_ops(P):
    """the ops of a plan that a keep_all binding runs as GEMM launches (every role)"""
    return [op for op in P.ops if op["live"] and op["kind"] in ("conv", "linear", "deconv") and not (op["kind"] == "deconv" and parse_op(op)[1]["cout"] == 1)]


def accepted_labels(P, tile):
    """labels of the ops under test `tile` runs; a follower goes with its op, so it must run too (followers are plain linears: every
    tile but the halo form takes them - the halo form's plan keeps none)"""
    return [op["label"] for op in P.ops if op["live"] and op["role"] == "test" and predicted_refusal(tile, op) is None]
