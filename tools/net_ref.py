"""float64 per-op reference of the mobile plans (plans/det.plan, plans/cls.plan, plans/rec.plan) as `Net(kind, precision="fp16")`
runs them - and a per-element error bound for every op, derived from the rounding points of the kernel that runs it.  Modelled on
tools/srv_ref.py (whose helpers it imports); `Ref.op` evaluates ONE op on caller-given inputs (tid -> f64 NHWC: the device's own
tensors, or the oracle's) and returns (reference, bound); bound None: the op is exact.  `ratio` <= 1 passes.

Weights (`Ref.__init__`): the LAB fold of DESIGN.md section 4 / net.hip fold_lab restated here - per conv / depthwise conv whose stage
list is  bias b | smul s0 | sadd a0 [| hswish | smul s1 | sadd a1]:  w' = f32(f64(w) s0 s_in), b' = f32(s0 (b + a_in sum_k w) + a0)
(double, k ascending), stages  bias b' [| hsw6: u = y clamp(y + 3, 0, 6) [| sfma: fma(u, s6, a1), s6 = f32(s1 / 6)]];  (s_in, a_in) is
the (s6, a1) of a depthwise conv with the full chain whose only reader is this 1x1 stride-1 conv (ABSORPTION: that depthwise conv
stops after hsw6).  half=True: the weights of the matrix products (dense convs with Cin != 3, linears on f16 tensors, the 24 -> 24
transposed conv) are then rounded to f16 (net.hip frag_to_half); depthwise taps, the stem, the SE fcs, the row-sum convs' image, the
DB head's fused form, the 24 -> 1 transposed conv, the classifier's pool -> fc and every parameter vector stay f32.  half=False: no
weight is rounded - the fp32 contract's values.

Notation: u16 = 2^-11, u32 = 2^-24, sub = 2^-25 (srv_ref).  Every kernel but the matrix products is the f32 kernel's source compiled
with f16 loads (exact) and ONE saturating, rounding store (conv_device.h ld4 / st4 / ld1 / st1): its f32 chain is the oracle's, so
the terms below are those of oracle_net.cpp's operations, one u32 |v| per rounded f32 result v, carried through the stages that
follow (`_stages`: a stage's Lipschitz constant times the error so far, plus its own rounding).  Terms per op kind:

  conv / linear / deconv (conv_mfma_kernel, conv_mfma_mt16_kernel, conv3x3_tile16_kernel; stem_kernel and dw kernels in f32): f16 x
      f16 products are exact in f32, the f32 sum over K (taps x channels padded to 8) in any order: K u32 sum|a w|; then the stages.
  stages: bias / sadd / addt / addup: u32 |y|.  bn: y s then + t, two roundings.  sfma: one.  mulc: u32 |y|.  relu: none.
      hsw6: t = clamp(y + 3, 0, 6) (u32 |y + 3| inside the clamp), u = y t (u32 |u|), local Lipschitz constant |t| + |y| [inside].
      hswish (not folded: the classifier): hsw6 then the IEEE quotient u / 6.  swish / sigmoid: e = ocr_expf(-y) (EXP_REL), d = 1 + e,
      y / d or 1 / d: one rounding each.  hsig (the SE gate): y slope + offset (two roundings), clamp.
  store: f16 tensors  u16 |y| + sub  after the clamp to +-65504;  f32 outputs (pool vectors, gates, the probability map, logits,
      probabilities): nothing more - the last stage's u32 |y| is the store's.
  gap (gap_rows_kernel + column pass): rows left to right, then the rows' sums top to bottom, one division: (W + H) u32 mean|x| + u32 |y|.
  sefc: two fma chains (C and C / 4 terms) with bias, relu between, hsig behind - as the conv terms, the hidden error through |W2|.
  pool: max exact; avg: kh kw u32 sum|x| / cnt + u32 |y|, the divisor is the number of window elements INSIDE the map (the
      recognizer at H = 28: the 3-row window on a 2-row map divides by 2 x 2; oracle/graph_ref.py states the same quirk).
  ln: srv_ref.Ref.ln_stats (two sequential f32 passes) and its bound.   concat: exact.
  attn (one thread per query, the oracle's order): q = x scale (u32), logit chain over hd = 15 ((hd + 1) u32 sum|q k|), s - m (u32),
      ocr_expf (EXP_REL), the sum over T keys and the division ((T + 2) u32), P V chain (T u32):
      bound = (2.02 E + (2 T + 4) u32) sum_j P_j |v_j| + store, E = max_j u32 ((hd + 1) sum|q k| + |s_j| + |m|) + EXP_REL.
  softmax (groups of 128 columns, two chains per group, groups folded in order - DESIGN.md section 4): per column the argument's
      u32 |x - M| and EXP_REL; the sum of positive terms keeps the largest relative error of its terms + (66 + G + 2) u32:
      bound = p (2 E + (70 + G) u32), E = max_c u32 |x_c - M| + EXP_REL.
  EXP_REL = 4 u32: ocr_expf is the Cephes expf (range reduction by two fmas, degree-5 Horner), whose stated peak relative error
      is 1.7e-7 = 2.9 u32; tests/test_net_ref.py sweeps the oracle's ocr_expf against exp in float64.  No approximate hardware
      instruction (v_rcp, v_exp, v_rsq) is on this path: `/` and sqrt are IEEE in these kernels (compiled with correctly rounded
      division; the CDNA ISA gives v_rcp_f32 / v_exp_f32 1 ulp, which EXP_REL and the u32 per
      division above would also cover), so no constant is taken for them.
  The three constants that are not a count of roundings, each derived:
      SECOND = 1 + 2^-10 on the carried error: k roundings in a row give (1 + u32)^k - 1 <= k u32 (1 + k u32); the longest chain of
      these plans has k < 9 x 960 + 32 < 2^14 roundings (the recognizer's 1 x 3 conv over 960 channels and its stages), so k u32 < 2^-10
      and the first-order sum times SECOND covers the products of roundings.
      1.001 in swish / sigmoid: the quotient by d = 1 + e with |dd| error of d is 1 / (d - dd) <= (1 / d)(1 + 1.001 dd / d) while
      dd / d <= 1e-3 - dd / d is at most EXP_REL + u32 + the carried error, and a carried error above 1e-3 fails the ratio anyway.
      2.02 in attn (as srv_ref): a weight P_j = p_j / l with relative errors <= E in p_j and in l is off by (1 + E) / (1 - E) - 1
      <= 2.02 E for E <= 0.0099; E here is below 1e-4.
  Row maxima: attn's E and softmax's E are the maximum over ONE row's keys / columns of the per-term relative error.  This is error
      propagation, not a tolerance scaled by a tensor's size: the denominator l is the sum of all the row's positive terms, so its
      relative error is bounded by the largest relative error among exactly those terms, and every output of the row divides by l.

Fused launches (the production list, keep_all = 0 / 2) - `Ref.composed` evaluates the group on its nearest existing inputs, the
missing tensor in f64, its error a term of the bound carried through the reader (|W| for a product, the gate for mulc, the mean
for gap).  Rounding points against the unfused pair's (`FUSIONS`):
  gate: SE gate folded into the reading 1x1 conv - NOT identical: the operand is f16(x f16(g)) (two packed f16 multiplies on the gate
      rounded to f16, conv_mfma_kernel) where ew_kernel stores f16(f32(x g)): 2 u16 |x g| + sub (1 + |x|) on the operand.
  dwpw: depthwise -> 1x1 - the same points (the depthwise half's u = hsw6 is clamped and rounded to f16 on its way to the matrix
      pipe, as the store would), but the 1x1 half is v_mfma_f32_32x32x8_f16 inside the block where the unfused conv may be the
      32x32x16 kernel: another order of the f32 sum, so not the same bits.
  xdw: expand 1x1 -> depthwise - f32 only (Net::plan_xdw refuses precision fp16): never runs in this mode.
  db_head: deconv 24 -> 24 + bn + relu -> deconv 24 -> 1 + sigmoid - NOT identical: the fused kernel keeps f32 weights and the
      24-channel value in f32 registers (db_head_mfma_kernel: f32 matrix instructions); unfused, f16 weights and an f16 tensor.
  cat: concat folded into the 3x3 conv's tile fill (conv3x3_tile16_kernel) - IDENTICAL points, the fill copies halfs (same kernel; the
      same bits only on the same input bits - in the detector its four sources come out of the RSE blocks, which the production
      list fuses, so the keep_all = 1 and 2 tensors differ there while both stay within the same bound).
  rowsum: the RSE blocks' conv 1x1 (K <= 24) run twice - NOT identical: first conv_rowsum_kernel (f32 weight image, f32 chain) leaves
      the pool's row sums of the UNROUNDED values, then the conv with x g + x [+ upsampled] in its epilogue on the unrounded
      accumulator (f16 weights); likewise a depthwise conv that leaves its row sums (dw..._rowsum) sums what it has before the
      store's rounding: the pool's reference on the stored tensor gets u16 |x| + sub per element, through the mean.
  ctc_head: linear -> softmax with only (arg max, max probability) kept - Net::dense_fused_head takes it only when the handle has
      arg-max / probability outputs (head_amax_ / head_pmax_), which the Rec stage sets and ocr_net_* does not; every fp16 rec case
      of tests/golden/net_launch_lists.json accordingly ends in `linear1x1_120_6625` and `softmax_6625`, the two launches checked here.

MUTATIONS: six local errors the checker must reject (tests/test_net_ref.py on the oracle's tensors, tests/test_gpu_net_ops.py on
the device's)."""
import numpy as np

from srv_ref import F16_MAX, SUB, U16, U32, f16, gi, parse_plan, ratio  # noqa: F401  (f16, ratio: re-exported for the tests)
from srv_ref import Ref as _SrvRef

EXP_REL = 4 * U32
SECOND = 1.0 + 2.0 ** -10
MUTATIONS = ("dw_halo_right_zero", "drop_granule_last_tap", "drop_last_bias", "gate_row_prev_image", "ln_unbiased", "avg_full_window")
# fusion -> do its rounding points (and its bits) equal the unfused launches'?
FUSIONS = {"gate": False, "dwpw": False, "xdw": None, "db_head": False, "cat": True, "rowsum": False, "ctc_head": None}


def _f32(a):
    return np.asarray(a, np.float32)


def _ceil8(c):
    return (c + 7) // 8 * 8


class Ref:
    def __init__(self, plan_text, params, half=True):
        self.ops = parse_plan(plan_text)
        self.half = half
        self.P = params
        self.out_tid = [gi(op, "i") for op in self.ops if op["kind"] == "output"][0]
        self.by_out = {gi(op, "o"): op for op in self.ops if op["kind"] != "output"}
        # storage (net.hip Net::load): plain f32 = softmax in / out and the probability map; f32 vectors = gap / sefc and ew on them
        self.f32_t = {0}
        for op in self.ops:
            k = op["kind"]
            if k == "softmax":
                self.f32_t |= {gi(op, "i"), gi(op, "o")}
            elif k == "deconv" and gi(op, "cout") == 1:
                self.f32_t.add(gi(op, "o"))
            elif k in ("gap", "sefc") or (k == "ew" and gi(op, "i") in self.f32_t):
                self.f32_t.add(gi(op, "o"))
        self._fold()

    def p(self, name):
        return _f32(self.P[name])

    # ----------------------------------------------------------------------------------------------------------- weights
    def _fold(self):
        ops = self.ops
        uses = {}
        for op in ops:
            if op["kind"] == "output":
                continue
            for t in (op["ins"] if op["kind"] == "concat" else [gi(op, "i")]):
                uses[t] = uses.get(t, 0) + 1
            for k, a in op["ep"]:
                if k in ("mulc", "addt", "addup"):
                    uses[int(a[0])] = uses.get(int(a[0]), 0) + 1
        lab = {}
        for i, op in enumerate(ops):
            e = [k for k, _ in op["ep"]]
            if op["kind"] not in ("conv", "dw"):
                continue
            p3 = e[:3] == ["bias", "smul", "sadd"]
            p6 = p3 and len(e) == 6 and e[3] == "act" and op["ep"][3][1][0] == "hswish" and e[4:] == ["smul", "sadd"]
            if not (p6 or (p3 and len(e) == 3)):
                continue
            sc = lambda j: float(self.p(op["ep"][j][1][0]).reshape(-1)[0])
            lab[i] = dict(s0=sc(1), a0=sc(2), act=p6, s1=sc(4) if p6 else 1.0, a1=sc(5) if p6 else 0.0)
        s6 = lambda s1: float(np.float32(np.float64(np.float32(s1)) / 6.0))
        absorbs, handed = {}, set()
        for i, d in enumerate(ops):
            if d["kind"] != "dw" or i not in lab or not lab[i]["act"] or gi(d, "o") == self.out_tid or uses.get(gi(d, "o"), 0) != 1:
                continue
            for j in range(i + 1, len(ops)):
                c = ops[j]
                if c["kind"] in ("concat", "output") or "i" not in c["kv"] or gi(c, "i") != gi(d, "o"):
                    continue
                if c["kind"] == "conv" and j in lab and all(gi(c, q) == v for q, v in (("kh", 1), ("kw", 1), ("sh", 1), ("sw", 1), ("ph", 0), ("pw", 0))):
                    absorbs[j] = i
                    handed.add(i)
                break
        for i, op in enumerate(ops):
            k = op["kind"]
            if k not in ("conv", "dw", "linear", "deconv"):
                continue
            W = self.p(op["kv"]["w"])
            st = []
            if i in lab:
                L = lab[i]
                b = self.p(op["ep"][0][1][0]).reshape(-1)
                s_in, a_in = (s6(lab[absorbs[i]]["s1"]), lab[absorbs[i]]["a1"]) if i in absorbs else (1.0, 0.0)
                Wd = W.astype(np.float64)
                ssum = np.cumsum(Wd.reshape(len(b), -1), axis=1)[:, -1] if i in absorbs else np.zeros(len(b))
                bf = (np.float64(L["s0"]) * (b.astype(np.float64) + np.float64(a_in) * ssum) + np.float64(L["a0"])).astype(np.float32)
                W = ((Wd * np.float64(L["s0"])) * np.float64(s_in)).astype(np.float32)
                st.append(("bias", bf.astype(np.float64)))
                if L["act"]:
                    st.append(("hsw6",))
                    if i not in handed:
                        st.append(("sfma", s6(L["s1"]), float(np.float32(L["a1"]))))
            else:
                for kk, a in op["ep"]:
                    if kk == "bias":
                        st.append(("bias", self.p(a[0]).reshape(-1).astype(np.float64)))
                    elif kk in ("smul", "sadd"):
                        st.append((kk, float(self.p(a[0]).reshape(-1)[0])))
                    elif kk == "bn":
                        g, be, m, v = (self.p(n).reshape(-1) for n in a[:4])
                        inv = np.float32(1.0) / np.sqrt(v + np.float32(float(a[4])))
                        st.append(("bn", (g * inv).astype(np.float64), (be - (m * inv) * g).astype(np.float64)))
                    elif kk == "act":
                        st.append(("act", a[0]))
                    elif kk in ("mulc", "addt"):
                        st.append((kk, int(a[0])))
                    elif kk == "addup":
                        st.append((kk, int(a[0]), int(a[1])))
                    else:
                        raise ValueError(kk)
            op["st"] = st
            op["W32"] = W.astype(np.float64)
            matrix = (k == "conv" and gi(op, "cin") != 3) or (k == "linear" and gi(op, "i") not in self.f32_t) or (k == "deconv" and gi(op, "cout") != 1)
            op["W16"] = W.astype(np.float16).astype(np.float64) if (self.half and matrix) else op["W32"]
        for op in ops:
            if op["kind"] == "ew":
                op["st"] = [(kk, int(a[0])) if kk != "addup" else (kk, int(a[0]), int(a[1])) for kk, a in op["ep"]]

    # ----------------------------------------------------------------------------------------------------------- stages
    def _stages(self, st, y, e, t, mut=None, din=None):
        """the f32 epilogue chain on y with the error e so far: (y, e).  din: errors of the tensors the stages read"""
        mut, din = mut or {}, din or {}
        up2 = lambda a, u: np.repeat(np.repeat(a, u, 1), u, 2)
        for s in st:
            k = s[0]
            if k == "bias":
                b = s[1]
                if mut.get("drop_last_bias"):
                    b = b.copy()
                    b[-1] = 0.0
                y = y + b
                e = e + U32 * np.abs(y)
            elif k == "sadd":
                y = y + s[1]
                e = e + U32 * np.abs(y)
            elif k == "smul":
                y = y * s[1]
                e = e * abs(s[1]) + U32 * np.abs(y)
            elif k == "sfma":
                y = y * s[1] + s[2]
                e = e * abs(s[1]) + U32 * np.abs(y)
            elif k == "bn":
                y = y * s[1]
                e = e * np.abs(s[1]) + U32 * np.abs(y)
                y = y + s[2]
                e = e + U32 * np.abs(y)
            elif k == "hsw6" or (k == "act" and s[1] == "hswish"):
                inside = (y + 3.0 > -e) & (y + 3.0 < 6.0 + e)
                c = np.clip(y + 3.0, 0.0, 6.0)
                ec = np.where(inside, e + U32 * np.abs(y + 3.0), 0.0)
                u = y * c
                e = e * c + np.abs(y) * ec + e * ec + U32 * np.abs(u)
                y = u
                if k == "act":  # (the IEEE quotient)
                    y = y / 6.0
                    e = e / 6.0 + U32 * np.abs(y)
            elif k == "act" and s[1] == "relu":
                y = np.maximum(y, 0.0)
            elif k == "act" and s[1] in ("swish", "sigmoid"):
                ex = np.exp(-np.clip(y, -88.0, 87.0))
                de = ex * (np.expm1(np.minimum(e, 1.0)) + EXP_REL)
                d = 1.0 + ex
                dd = de + U32 * d
                num = y if s[1] == "swish" else np.ones_like(y)
                out = num / d
                e = np.abs(out) * (dd / d * 1.001 + U32) + (e / d if s[1] == "swish" else 0.0)
                y = out
            elif k == "mulc":
                g = t[s[1]]
                if mut.get("gate_row_prev_image") and g.shape[0] > 1:  # image n reads the gate row of image n - 1
                    g = np.concatenate([g[:1], g[:-1]], 0)
                eg = din.get(s[1], 0.0)
                y2 = y * g
                e = e * np.abs(g) + np.abs(y) * eg + U32 * np.abs(y2)
                y = y2
            elif k == "addt":
                y = y + t[s[1]]
                e = e + din.get(s[1], 0.0) + U32 * np.abs(y)
            elif k == "addup":
                y = y + up2(t[s[1]], s[2])
                e = e + (up2(din[s[1]], s[2]) if s[1] in din else 0.0) + U32 * np.abs(y)
            else:
                raise ValueError(s)
        return y, e

    def _store(self, op, y, e, rounded=True):
        """the store: f16 tensors clamp and round once; f32 outputs keep the chain's last rounding"""
        e = e * SECOND
        if self.half and rounded and gi(op, "o") not in self.f32_t:
            y = np.clip(y, -F16_MAX, F16_MAX)
            return y, e + U16 * np.abs(y) + SUB
        return y, e

    # ----------------------------------------------------------------------------------------------------------- products
    @staticmethod
    def _cols(x, kh, kw, sh, sw, ph, pw):
        n, h, w, c = x.shape
        oh, ow = (h + 2 * ph - kh) // sh + 1, (w + 2 * pw - kw) // sw + 1
        xp = np.pad(x, ((0, 0), (ph, ph), (pw, pw), (0, 0)))
        cols = np.empty((n, oh, ow, kh, kw, c))
        for y in range(kh):
            for xx in range(kw):
                cols[:, :, :, y, xx] = xp[:, y:y + sh * (oh - 1) + 1:sh, xx:xx + sw * (ow - 1) + 1:sw]
        return cols

    def _product(self, op, x, W, dx=None, mut=None):
        """(acc, err): the product and K u32 sum|a w| + |W| dx"""
        mut = mut or {}
        k = op["kind"]
        if k == "dw":
            kh, kw = gi(op, "kh"), gi(op, "kw")
            geo = [gi(op, q) for q in ("kh", "kw", "sh", "sw", "ph", "pw")]
            cols = self._cols(x, *geo)  # [n, oh, ow, kh, kw, c]
            if mut.get("dw_halo_right_zero"):  # 16-pixel tiles: the last column's right-most tap reads zero where the map goes on
                cols = cols.copy()
                ow, wi = cols.shape[2], x.shape[2]
                for ox in range(15, ow, 16):
                    if ox * geo[3] - geo[5] + kw - 1 < wi:
                        cols[:, :, ox, :, kw - 1] = 0.0
            Wt = W[:, 0].transpose(1, 2, 0)  # [kh, kw, c]
            acc = (cols * Wt).sum((3, 4))
            S = (np.abs(cols) * np.abs(Wt)).sum((3, 4))
            err = kh * kw * U32 * S
            if dx is not None:
                err = err + (self._cols(dx, *geo) * np.abs(Wt)).sum((3, 4))
            return acc, err
        if k == "conv":
            geo = [gi(op, q) for q in ("kh", "kw", "sh", "sw", "ph", "pw")]
            if mut.get("drop_granule_last_tap"):
                W = W.copy()
                W[:, 0:8, -1, -1] = 0.0
            cols = self._cols(x, *geo)
            n, oh, ow = cols.shape[:3]
            A = cols.reshape(n * oh * ow, -1)
            Wm = W.transpose(2, 3, 1, 0).reshape(-1, W.shape[0])
            K = geo[0] * geo[1] * (3 if W.shape[1] == 3 else _ceil8(W.shape[1]))  # (the stem's chain has no padded channels)
            shp = (n, oh, ow, -1)
            dA = None if dx is None else self._cols(dx, *geo).reshape(n * oh * ow, -1)
        elif k == "linear":
            n, h, w, c = x.shape
            A, Wm, K, shp = x.reshape(-1, c), W, _ceil8(c), (n, h, w, -1)
            dA = None if dx is None else dx.reshape(-1, c)
        else:  # deconv: [N, H, W, 4 (dy, dx), cout]
            n, h, w, c = x.shape
            co = W.shape[1]
            A, Wm, K, shp = x.reshape(-1, c), W.transpose(0, 2, 3, 1).reshape(c, 4 * co), _ceil8(c), (n, h, w, 4, co)
            dA = None if dx is None else dx.reshape(-1, c)
        acc = A @ Wm
        err = K * U32 * (np.abs(A) @ np.abs(Wm))
        if dA is not None:
            err = err + dA @ np.abs(Wm)
        return acc.reshape(shp), err.reshape(shp)

    @staticmethod
    def _untap(a):
        n, h, w, _, co = a.shape
        return a.reshape(n, h, w, 2, 2, co).transpose(0, 1, 3, 2, 4, 5).reshape(n, 2 * h, 2 * w, co)

    # ----------------------------------------------------------------------------------------------------------- ops
    def op(self, op, t, mut=None, din=None, w16=True, rounded=True):
        """(reference, bound) of one op on the tensors t.  din: tid -> per-element error of an input that is itself a reference
        (`composed`); w16=False: the f32 weights (the kernels that keep them); rounded=False: the value stays in f32 registers"""
        k = op["kind"]
        din = din or {}
        if k in ("conv", "linear", "deconv", "dw"):
            x = t[gi(op, "i")]
            acc, e = self._product(op, x, op["W16"] if w16 else op["W32"], din.get(gi(op, "i")), mut)
            if k == "deconv":
                acc, e = self._untap(acc), self._untap(e)
            y, e = self._stages(op["st"], acc, e, t, mut, din)
            return self._store(op, y, e, rounded)
        if k == "ew":
            x = t[gi(op, "i")]
            y, e = self._stages(op["st"], x, din.get(gi(op, "i"), np.zeros_like(x)), t, mut, din)
            return self._store(op, y, e, rounded)
        if k == "gap":
            x = t[gi(op, "i")]
            n, h, w, c = x.shape
            y = x.mean((1, 2), keepdims=True)
            e = (w + h) * U32 * np.abs(x).mean((1, 2), keepdims=True) + U32 * np.abs(y)
            if gi(op, "i") in din:
                e = e + din[gi(op, "i")].mean((1, 2), keepdims=True)
            return y, e * SECOND
        if k == "sefc":
            return self.sefc(op, t[gi(op, "i")], din.get(gi(op, "i")))
        if k == "concat":
            return np.concatenate([np.repeat(np.repeat(t[i], u, 1), u, 2) for i, u in zip(op["ins"], op["ups"])], -1), None
        if k == "pool":
            return self.pool(op, t[gi(op, "i")], mut)
        if k == "ln":
            return self.ln(op, t[gi(op, "i")], mut)
        if k == "attn":
            return self.attn(op, t[gi(op, "i")])
        if k == "softmax":
            return self.softmax(t[gi(op, "i")])
        raise ValueError(k)

    def sefc(self, op, m, dm=None):
        C, R = gi(op, "c"), gi(op, "cr")
        w1 = self.p(op["kv"]["w1"]).reshape(R, C).astype(np.float64)
        w2 = self.p(op["kv"]["w2"]).reshape(C, R).astype(np.float64)
        b1, b2 = (self.p(op["kv"][q]).reshape(-1).astype(np.float64) for q in ("b1", "b2"))
        slope, offset = float(np.float32(op["kv"]["slope"])), float(np.float32(op["kv"]["offset"]))
        v = m.reshape(-1, C)
        a = v @ w1.T
        e = C * U32 * (np.abs(v) @ np.abs(w1.T)) + (0.0 if dm is None else dm.reshape(-1, C) @ np.abs(w1.T))
        h = a + b1
        e = e + U32 * np.abs(h)
        h = np.maximum(h, 0.0)
        a2 = h @ w2.T
        e2 = R * U32 * (h @ np.abs(w2.T)) + e @ np.abs(w2.T)
        z = a2 + b2
        e2 = e2 + U32 * np.abs(z)
        z = z * slope
        e2 = e2 * abs(slope) + U32 * np.abs(z)
        z = z + offset
        e2 = e2 + U32 * np.abs(z)
        shp = m.shape[:3] + (C,)
        return np.clip(z, 0.0, 1.0).reshape(shp), (e2 * SECOND).reshape(shp)

    def pool(self, op, x, mut=None):
        kh, kw, sh, sw = (gi(op, q) for q in ("kh", "kw", "sh", "sw"))
        n, h, w, c = x.shape
        oh, ow = int((h - kh) / sh) + 1, int((w - kw) / sw) + 1  # C++ truncation: a 3-row window on a 2-row map is one output row
        mx = op["kv"]["type"] == "max"
        acc = np.full((n, oh, ow, c), -np.inf) if mx else np.zeros((n, oh, ow, c))
        sab, cnt = np.zeros((n, oh, ow, c)), np.zeros((1, oh, ow, 1))
        for oy in range(oh):
            for ox in range(ow):
                win = x[:, oy * sh:min(oy * sh + kh, h), ox * sw:min(ox * sw + kw, w)]
                if mx:
                    acc[:, oy, ox] = win.max((1, 2))
                else:
                    acc[:, oy, ox] = win.sum((1, 2))
                    sab[:, oy, ox] = np.abs(win).sum((1, 2))
                cnt[0, oy, ox, 0] = win.shape[1] * win.shape[2]
        if mx:
            return acc, None
        if (mut or {}).get("avg_full_window"):
            cnt = np.full_like(cnt, kh * kw)
        y = acc / cnt
        return self._store(op, y, kh * kw * U32 * sab / cnt + U32 * np.abs(y))

    def ln(self, op, x, mut=None):
        g = self.p(op["kv"]["g"]).astype(np.float64)
        b = self.p(op["kv"]["b"]).astype(np.float64)
        m, r, dm, dr = _SrvRef.ln_stats(x, float(np.float32(op["kv"]["eps"])), unbiased=(mut or {}).get("ln_unbiased", False))
        y = (x - m) * r * g + b
        e = np.abs(g) * r * (dm + np.abs(x - m) * (dr + 4 * U32)) + 2 * U32 * np.abs(b) + U32 * np.abs(y)
        return self._store(op, y, e)

    def attn(self, op, x):
        heads, hd = gi(op, "heads"), gi(op, "hd")
        scale = float(np.float32(op["kv"]["scale"]))
        n, h, w, _ = x.shape
        T, D = h * w, heads * hd
        q, k, v = x.reshape(n, T, 3, heads, hd).transpose(2, 0, 3, 1, 4)
        q = q * scale
        S = q @ k.transpose(0, 1, 3, 2)
        Sa = np.abs(q) @ np.abs(k.transpose(0, 1, 3, 2))
        m = S.max(-1, keepdims=True)
        p = np.exp(S - m)
        P = p / p.sum(-1, keepdims=True)
        o = P @ v
        E = (U32 * ((hd + 1) * Sa + np.abs(S) + np.abs(m))).max(-1, keepdims=True) + EXP_REL
        e = (2.02 * E + (2 * T + 4) * U32) * (P @ np.abs(v))
        tr = lambda a: a.transpose(0, 2, 1, 3).reshape(n, h, w, D)
        return self._store(op, tr(o), tr(e))

    def softmax(self, x):
        C = x.shape[-1]
        M = x.max(-1, keepdims=True)
        p = np.exp(x - M)
        y = p / p.sum(-1, keepdims=True)
        E = (U32 * np.abs(x - M)).max(-1, keepdims=True) + EXP_REL
        return y, y * (2 * E + (70 + (C + 127) // 128) * U32) * SECOND

    # ----------------------------------------------------------------------------------------------------------- fused launches
    def composed(self, tid, t, exists, rowsum=True):
        """(reference, bound, fusions) of tensor `tid` of a production-list run on its nearest EXISTING inputs (t: the existing
        tensors): a missing input is evaluated in f64 from its own inputs, its error a term of the bound.  fusions: the names of
        FUSIONS met on the way (empty: an ordinary launch)"""
        op = self.by_out[tid]
        tt, din, met = dict(t), {}, []
        k = op["kind"]
        w16, rounded = True, True

        def need(i, reader):
            if i == 0 or exists(i):
                return
            src = self.by_out[i]
            sk = src["kind"]
            for j in (src["ins"] if sk == "concat" else [gi(src, "i")]) + [s[1] for s in src.get("st", []) if s[0] in ("mulc", "addt", "addup")]:
                need(j, src)
            if sk == "concat":
                tt[i] = self.op(src, tt)[0]
                din[i] = np.concatenate([np.repeat(np.repeat(din.get(a, np.zeros_like(tt[a])), u, 1), u, 2) for a, u in zip(src["ins"], src["ups"])], -1)
                met.append("cat")
            elif sk == "ew":  # the folded gate: f16(x f16(g)) against x g
                x, g = tt[gi(src, "i")], tt[src["st"][0][1]]
                assert len(src["st"]) == 1 and src["st"][0][0] == "mulc", src
                tt[i] = x * g
                din[i] = 2 * U16 * (1 + U16) * np.abs(tt[i]) + SUB * (1.0 + np.abs(x)) + np.abs(x) * din.get(src["st"][0][1], 0.0)
                met.append("gate")
            elif sk == "dw":
                tt[i], din[i] = self.op(src, tt, din=din)
                met.append("dwpw")
            elif sk == "deconv":  # the fused DB head: f32 weights, the value stays in registers
                tt[i], din[i] = self.op(src, tt, din=din, w16=False, rounded=False)
                met.append("db_head")
            elif sk == "conv":  # the RSE block's conv: row-sum pass (f32 image) for the pool, second pass (f16 fragments) for the ew
                tt[i], din[i] = self.op(src, tt, din=din, w16=reader["kind"] != "gap", rounded=False)
                met.append("rowsum")
            else:
                raise ValueError("no fused launch leaves a %s tensor out" % sk)

        ins = (op["ins"] if k == "concat" else [gi(op, "i")]) + [s[1] for s in op.get("st", []) if s[0] in ("mulc", "addt", "addup")]
        for i in ins:
            need(i, op)
        if k == "gap" and rowsum and exists(gi(op, "i")) and self.by_out[gi(op, "i")]["kind"] == "dw" and self.half:
            x = tt[gi(op, "i")]  # a depthwise conv that leaves its row sums adds them before its store rounds
            din[gi(op, "i")] = U16 * np.abs(x) + SUB
            met.append("rowsum")
        if k == "deconv" and gi(op, "cout") == 1 and "db_head" in met:
            w16 = False
        y, b = self.op(op, tt, din=din, w16=w16, rounded=rounded)
        return y, b, met


def kind_of(op):
    k = op["kind"]
    if k == "conv":
        return "stem" if gi(op, "cin") == 3 else "conv%dx%d" % (gi(op, "kh"), gi(op, "kw"))
    if k == "dw":
        return "dw%dx%d" % (gi(op, "kh"), gi(op, "kw"))
    if k == "deconv":
        return "deconv_map" if gi(op, "cout") == 1 else "deconv"
    if k == "pool":
        return "pool_" + op["kv"]["type"]
    return k


def mutation_site(ref, mut, t):
    """the op a mutation is applied to on the tensors t (None: none of the plan's ops is changed by it at these shapes)"""
    for op in ref.ops:
        k = op["kind"]
        if k == "output" or gi(op, "o") not in t:
            continue
        if mut == "dw_halo_right_zero" and k == "dw" and gi(op, "kh") == 5 and gi(op, "sw") == 1 and t[gi(op, "o")].shape[2] >= 18:
            return op
        if mut == "drop_granule_last_tap" and k == "conv" and gi(op, "kh") == 3 and gi(op, "kw") == 3 and gi(op, "cin") >= 8:
            return op
        if mut == "drop_last_bias" and k in ("conv", "linear") and gi(op, "cin") != 3 and op["st"] and op["st"][0][0] == "bias" and abs(op["st"][0][1][-1]) >= 0.02:
            return op
        if mut == "gate_row_prev_image" and k == "ew" and op["st"][0][0] == "mulc" and t[gi(op, "o")].shape[0] > 1:
            return op
        if mut == "ln_unbiased" and k == "ln":
            return op
        if mut == "avg_full_window" and k == "pool" and op["kv"]["type"] == "avg" and t[gi(op, "i")].shape[1] % gi(op, "sh"):
            return op
    return None


def check_tensors(ref, t, exists=None):
    """every op of the plan on the tensors t of one run (tid -> f64 NHWC, t[0] = the input): {tid: (kind, err / bound, fusions)};
    exists: the production list's `exists` - fused groups take the composed reference"""
    res = {}
    for op in ref.ops:
        if op["kind"] == "output" or gi(op, "o") not in t:
            continue
        o = gi(op, "o")
        if exists is None:
            y, b = ref.op(op, t)
            met = []
        else:
            y, b, met = ref.composed(o, t, exists)
        res[o] = ("+".join(sorted(set(met))) + ":" + kind_of(op) if met else kind_of(op), ratio(t[o], y, b), met)
    return res


def run_chain(ref, x):
    """the whole plan through the reference, every f16 tensor rounded as the device's store would (half=True): the emulated mode"""
    t = {0: np.asarray(x, np.float64)}
    for op in ref.ops:
        if op["kind"] == "output":
            continue
        y = ref.op(op, t)[0]
        o = gi(op, "o")
        if o in ref.f32_t:
            y = y.astype(np.float32).astype(np.float64)
        elif ref.half:
            y = f16(y)
        t[o] = y
    return t
