"""float64 per-op reference of the server plans (plans/srv_det.plan, plans/srv_rec.plan) - and a per-element error bound for every
op the device runs, derived from that kernel's own rounding points.

Two uses:
  * `torch_run`: the whole plan in float64 torch, written from the plan grammar alone (a second opinion on the oracle; the CPU
    suite compares the two).
  * `Ref`: ONE op at a time in float64 numpy on caller-given inputs - the device's own f16 (or f32) tensors - with the weights
    restated exactly as the f16 build stores them (srv_net.hip: batch norm folded into the weights, bias and shift one vector,
    rounded to f16; the absorbed LayerNorm's diag(gamma) W1, s and c).  `check` returns max |got - ref| / bound; an op passes at
    <= 1.  The bound never looks at a tensor's maximum: it is per element, so a wrong tile edge, one dropped bias column or a 0.3 %
    bias in a normalisation shows at the elements it touches (`MUTATIONS`: six such errors the checker must reject).

Notation: u16 = 2^-11 (f16 unit roundoff), u32 = 2^-24 (f32), sub = 2^-25 (half the f16 subnormal spacing: the absolute error of
one rounding to f16 near zero).  Rounding points, per op kind:

  GEMM (conv / linear / 2x2 transposed conv; f16 build): f16 x f16 products are exact in f32; the sum over K runs in f32 (any
  order: |error| <= K u32 sum_k |a_k w_k|); the epilogue adds the folded bias b and the residual r in f32 (2 u32 (|b| + |r|)),
  applies the activation (its Lipschitz constant L carries the error; GELU is the kernel's polynomial fit `gelu_fit`, evaluated
  in f32: 16 u32 (|x| + 1e-30)), clamps to +-65504 and rounds once to f16 (u16 |y| + sub).  f32 outputs (map, logits): u32 |y|.
      bound = u_out |y| + sub + L (K u32 S + 2 u32 (|b| + |r|)) + act_eval,   S = sum_k |a_k w_k| in f64
  attention (attn_h_kernel): q scale log2(e) rounded to f16 (the reference uses that q, exactly), S = q k in f32 (32 u32
  sum_d |q_d k_d|), m subtracted (u32 |S - m|), hardware exp2 (2^-22 relative): per key a relative error eps_j of p_j =
  ln2 e_j + 2^-22; the max over the row's keys E; p rounded to f16 for P V (u16 + sub / p), the denominator sums the unrounded p;
  P V in f32 over n keys (n u32), O / l and one rounding (u16 |o| + sub):
      bound_d = (2.02 E + u16 + (n + 4) u32) sum_j P_j |v_jd| + sub sum_j |v_jd| / l + u16 |o_d| + sub
  LayerNorm (two passes, f32): the sum's error C u32 sum|x| (any order), the mean's dm = that / C + u32 |m|; the variance's relative
  error (C + 3) u32 + dm^2 / var, rstd's half of it + 2 u32; then (x - m) r g + b in f32 and the f16 rounding:
      bound = |g| r (dm + |x - m| (dr + 4 u32)) + 2 u32 |b| + u16 |y| + sub
  pool (max) / concat / pack: exact.  pool (avg) / addpos: one f32 rounding per add plus the f16 rounding.
  fused MLP (srv_mlp.h): fc1 as a GEMM, its hidden value rounded to f16 (that rounding is a term of the bound, the reference keeps
  the f64 value), fc2 over 4 C hidden units: bound = sum_k |w2_k| bound_h_k + 4 C u32 sum_k |h_k w2_k| + the epilogue as above.
  With the LayerNorm absorbed: fc1 = r (u W1') - r m s + c (the f32 sum has the GEMM error on u, not on u - m).  The statistics
  are allowed the error of one pass shifted by the row's first channel x0: var = E[(x - x0)^2] - (m - x0)^2, relative error
  (C + 3) u32 (1 + (m - x0)^2 / var).  The kernel's unshifted pass, E[x^2] - m^2 (srv_mlp.h), carries (1 + m^2 / var) instead:
  on a token whose channels share an offset of 300 sigma the rest of this bound - the f32 sum over u, carried through fc2 - is
  the larger term, so such rows do not separate the two forms.  The residual LN(u) is formed in f32, not rounded.
  head tail: the mid map relu(x W1 + b1) rounded to f16, the second product on f16 weights, sigmoid: 0.25 (sum |w4| bound_mid +
  64 u32 S2 + u32 |b2|) + 2^-21.
  CTC tail (`ctc_tail`: arg max = first maximum, p = 1 / sum_c exp(x_c - M), relative bounds on p).  A term's exponent is formed as
  (x - m) log2(e): the difference rounds (u32 |x - m|), the constant and the product round (2 u32 |x - m|), and the hardware exp2
  is good to 2^-22 = 4 u32 (CDNA ISA: v_exp_f32, 1 ulp): relative 3 u32 |x - m| + 4 u32.  A running sum that is rescaled when its
  maximum moves from m to m' takes the same again with |m - m'|, plus one product and one addition (2 u32); maxima only grow, so the
  differences along a term's path add up to |x - M| and only the count of rescales n matters.  A sum of positive terms keeps the
  largest relative error of its terms plus u32 per addition on a term's path.  1 / sum: 2 u32 (the IEEE quotient has 1, v_rcp_f32 2).
      two-pass (argmax_softmax_kernel, ocr_expf = EXP_REL 4 u32 on the f32 difference): u32 D + 4 u32 + (ceil(C / 64) + 6) u32 + 2 u32
      one-pass (argmax_softmax_fast_kernel): per step of 256 columns a lane rescales once (exp2 4 + product 1) and adds 4 terms (4);
          each of the 6 butterfly folds is one rescale, one product, one addition (6): 3 u32 D + 9 u32 ceil(C / 256) + 36 u32 + 2 u32
      fused head (the matrix kernel's ctc_part epilogue, then ctc_reduce_kernel; `ctc_head`): inside a partial of W columns (64, whatever the tile) a term takes
          one exp2 (4), at most W additions and at most 6 cross-lane rescales (6 each); then the fold over n tiles:
          3 u32 D + 4 u32 + W u32 + 36 u32 + 6 u32 n + 2 u32
      fold of partials (ctc_reduce_kernel on given (m_s, sum_s)): 3 u32 max_s |m_s - M| + (4 + 2) u32 n_slots + 2 u32
  with D = max_c |x_c - M| over the finite columns, all times SECOND = 1 + 2^-10 for the second-order terms.
"""
import math

import numpy as np

U16 = 2.0 ** -11
U32 = 2.0 ** -24
SUB = 2.0 ** -25
F16_MAX = 65504.0
LN2 = math.log(2.0)
LOG2E = 1.44269504088896341
# srv_kernels.hip srv_gelu8: gelu(x) = x / 2 + t^2 P(t^2) + (|x| - t) / 2, t = min(|x|, 4)
GELU_FIT = (2.27814575e-08, -1.59860303e-06, 4.79555300e-05, -8.14015556e-04, 8.77238884e-03, -6.45731141e-02, 3.97883359e-01)
GELU_FIT_ERR = 1.9e-4  # max |fit - exact GELU| the kernel's comment states (tests/test_server_plans.py checks it)
ACT_L = {"none": 1.0, "relu": 1.0, "gelu": 1.13, "hswish": 1.5, "sigmoid": 0.25}


# --------------------------------------------------------------------------------------------------------------- plans
def parse_plan(text):
    """the plan's ops in order: dict(kind, kv (str -> str), ep [(stage, [args])], ins, ups)"""
    ops = []
    for line in text.splitlines():
        if not line or line[0] == "#" or line.startswith("plan "):
            continue
        toks = line.split()
        kv = dict(tk.split("=", 1) for tk in toks[1:])
        op = dict(kind=toks[0], kv=kv, ep=[])
        for st in (kv.get("ep", "").split("|") if kv.get("ep") else []):
            k, _, a = st.partition(":")
            op["ep"].append((k, a.split(",")))
        if toks[0] == "concat":
            op["ins"] = [int(v) for v in kv["i"].split(",")]
            op["ups"] = [int(v) for v in kv["up"].split(",")]
        ops.append(op)
    return ops


def gi(op, k, d=0):
    return int(op["kv"].get(k, d))


def f16(a):
    """round to f16 as the device's stores do (clamp to +-65504, round to nearest even), back in f64"""
    return np.clip(np.asarray(a, np.float64), -F16_MAX, F16_MAX).astype(np.float32).astype(np.float16).astype(np.float64)


def gelu_fit(x):
    x = np.asarray(x, np.float64)
    t = np.minimum(np.abs(x), 4.0)
    t2 = t * t
    q = np.zeros_like(x)
    for c in GELU_FIT:
        q = q * t2 + c
    return 0.5 * x + t2 * q + 0.5 * (np.abs(x) - t)


def _act(name, y, half):
    """(activation of y, bound of its evaluation in f32)"""
    if name == "none":
        return y, 0.0
    if name == "relu":
        return np.maximum(y, 0.0), 0.0
    if name == "gelu":
        if half:
            return gelu_fit(y), 16 * U32 * (np.abs(y) + 1e-30)
        import torch
        g = torch.nn.functional.gelu(torch.from_numpy(y)).numpy()
        return g, 5e-7 * np.abs(y) + 8 * U32 * np.abs(g)  # ocr_erff within 5e-7 of erf
    if name == "hswish":
        h = y * np.clip(y + 3.0, 0.0, 6.0) / 6.0
        return h, 4 * U32 * np.abs(y)
    if name == "sigmoid":
        s = 1.0 / (1.0 + np.exp(-y))
        return s, s * (1 - s) * np.abs(y) * 2 * U32 + 8 * U32 * s
    raise ValueError(name)


# --------------------------------------------------------------------------------------------------------------- weights
class Ref:
    """per-op float64 reference of a server plan with the weights as the f16 build (half=True) or the f32 twin stores them"""

    def __init__(self, plan_text, params, half=True):
        self.ops = parse_plan(plan_text)
        self.half = half
        self.P = params
        self.out_tid = [gi(op, "i") for op in self.ops if op["kind"] == "output"][0]
        self.ln_fold = {}
        for k, op in enumerate(self.ops):
            if op["kind"] in ("conv", "linear", "deconv"):
                self._restate(op)
        for k in range(len(self.ops) - 1):
            l, f1 = self.ops[k], self.ops[k + 1]
            if l["kind"] == "ln" and f1["kind"] == "linear" and f1.get("act") == "gelu" and gi(f1, "i") == gi(l, "o"):
                self.ln_fold[k + 1] = self._restate_ln_fold(f1, l)

    def by_out(self, tid):
        for op in self.ops:
            if op["kind"] != "output" and gi(op, "o") == tid:
                return op
        raise KeyError(tid)

    def _restate(self, op):
        """srv_net.hip prepare_op in f32 numpy: inv = 1/sqrt(v+eps), s = g inv, W s and b s + (beta - m inv g), then f16"""
        P = self.P
        W = np.asarray(P[op["kv"]["w"]], np.float32)
        cout = gi(op, "cout")
        b = s = t = None
        op["act"], op["res"] = "none", None
        for k, a in op["ep"]:
            if k == "bias":
                b = np.asarray(P[a[0]], np.float32).reshape(-1)
            elif k == "bn":
                g, be, m, v = (np.asarray(P[n], np.float32).reshape(-1) for n in a[:4])
                inv = np.float32(1.0) / np.sqrt(v + np.float32(float(a[4])))
                s = g * inv
                t = be - (m * inv) * g
            elif k == "addt":
                op["res"] = (int(a[0]), 1)
            elif k == "addup":
                op["res"] = (int(a[0]), int(a[1]))
            elif k == "act":
                op["act"] = a[0]
        # per-output-channel scale along the cout axis of each layout: conv [co][ci][kh][kw], linear [ci][co], deconv [ci][co][2][2]
        shape = {"conv": (-1, 1, 1, 1), "linear": (1, -1), "deconv": (1, -1, 1, 1)}[op["kind"]]
        single = op["kind"] == "deconv" and cout == 1
        if self.half and not single:
            if s is not None:
                W = W * s.reshape(shape)
                b = (b * s if b is not None else np.zeros(cout, np.float32)) + t
                s = t = None
            W = W.astype(np.float16)
        op["W"] = W.astype(np.float64)
        op["b"] = None if b is None else b.astype(np.float64)
        op["s"] = None if s is None else s.astype(np.float64)
        op["t"] = None if t is None else t.astype(np.float64)

    def _restate_ln_fold(self, f1, l):
        """srv_net.hip prepare_ln_fold: W1' = f16(W1 * gamma) [ci][co], s = sum_c W1' (f64 -> f32), c = b1 + sum_c W1 beta (f64 -> f32)"""
        P = self.P
        W = np.asarray(P[f1["kv"]["w"]], np.float32)
        g = np.asarray(P[l["kv"]["g"]], np.float32).reshape(-1)
        be = np.asarray(P[l["kv"]["b"]], np.float32).reshape(-1)
        b1 = [np.asarray(P[a[0]], np.float32).reshape(-1) for k, a in f1["ep"] if k == "bias"][0]
        W1 = (W * g[:, None]).astype(np.float16).astype(np.float64)
        sv = W1.sum(0).astype(np.float32).astype(np.float64)
        cv = (b1.astype(np.float64) + W.astype(np.float64).T @ be.astype(np.float64)).astype(np.float32).astype(np.float64)
        return dict(W1=W1, s=sv, c=cv, g=g.astype(np.float64), b=be.astype(np.float64), eps=float(l["kv"]["eps"]))

    # ----------------------------------------------------------------------------------------------------------- ops
    def op(self, op, t, mut=None):
        """(reference, bound) of one op on the tensors t (tid -> f64 NHWC) - the values the op reads, as the device holds them.
        bound None: the op is exact (the result must equal the reference)."""
        k = op["kind"]
        if k in ("conv", "linear", "deconv"):
            if k == "deconv" and gi(op, "cout") == 1:
                return self.deconv_map(op, t[gi(op, "i")])
            return self.gemm(op, t, mut)
        if k == "pool":
            return self.pool(op, t[gi(op, "i")], mut)
        if k == "concat":
            if (mut or {}).get("concat_next_shift"):  # source j read at (y >> s, x >> s) with source j + 1's shift (clamped to its own extent)
                oh, ow = t[op["ins"][-1]].shape[1] * op["ups"][-1], t[op["ins"][-1]].shape[2] * op["ups"][-1]
                ups = op["ups"][1:] + op["ups"][-1:]
                return np.concatenate([t[i][:, np.minimum(np.arange(oh) // u, t[i].shape[1] - 1)][:, :, np.minimum(np.arange(ow) // u, t[i].shape[2] - 1)]
                                       for i, u in zip(op["ins"], ups)], -1), None
            return np.concatenate([np.repeat(np.repeat(t[i], u, 1), u, 2) for i, u in zip(op["ins"], op["ups"])], -1), None
        if k == "ew":
            return self.addpos(op, t[gi(op, "i")])
        if k == "ln":
            return self.ln(op, t[gi(op, "i")], mut)
        if k == "attn":
            return self.attn(op, t[gi(op, "i")], mut)
        raise ValueError(k)

    def _out_round(self, y, f32_out=False):
        if self.half and not f32_out:
            return U16 * np.abs(y) + SUB
        return U32 * np.abs(y)

    def _product(self, op, x, W=None, wrap_pad=False):
        """(acc, S = sum |a w|, K) of a conv / linear / deconv on NHWC x; deconv: [N, H, W, 4, cout] by tap (dy, dx).  wrap_pad (a
        mutation): a padding tap at the right or bottom border reads what lies at its address - pixel (iy W + ix) of the flattened
        image, the neighbouring row or the next image - instead of zero"""
        W = op["W"] if W is None else W
        k = op["kind"]
        cin_s = (gi(op, "cin") + 7) // 8 * 8
        if k == "linear":
            n, h, w, c = x.shape
            A = x.reshape(-1, c)
            return (A @ W).reshape(n, h, w, -1), (np.abs(A) @ np.abs(W)).reshape(n, h, w, -1), cin_s
        if k == "deconv":
            n, h, w, c = x.shape
            co = W.shape[1]
            Wm = W.transpose(0, 2, 3, 1).reshape(c, 4 * co)
            A = x.reshape(-1, c)
            return (A @ Wm).reshape(n, h, w, 4, co), (np.abs(A) @ np.abs(Wm)).reshape(n, h, w, 4, co), cin_s
        kh, kw, sh, sw, ph, pw = (gi(op, q) for q in ("kh", "kw", "sh", "sw", "ph", "pw"))
        n, h, w, c = x.shape
        xp = np.pad(x, ((0, 0), (ph, ph), (pw, pw), (0, 0)))
        if wrap_pad:
            flat = np.concatenate([x.reshape(-1, c), np.zeros(((ph + 1) * w + pw + 1, c))])
            iy, ix = np.arange(-ph, h + ph)[:, None], np.arange(-pw, w + pw)[None, :]
            past = ((ix >= w) & (iy >= 0) & (iy < h)) | ((iy >= h) & (ix >= 0) & (ix < w))
            for k in range(n):
                xp[k][past] = flat[(k * h * w + iy * w + ix)[past]]
        oh, ow = (h + 2 * ph - kh) // sh + 1, (w + 2 * pw - kw) // sw + 1
        cols = np.empty((n, oh, ow, kh, kw, c))
        for y in range(kh):
            for xx in range(kw):
                cols[:, :, :, y, xx] = xp[:, y:y + sh * (oh - 1) + 1:sh, xx:xx + sw * (ow - 1) + 1:sw]
        A = cols.reshape(n * oh * ow, -1)
        Wm = W.transpose(2, 3, 1, 0).reshape(-1, W.shape[0])
        return (A @ Wm).reshape(n, oh, ow, -1), (np.abs(A) @ np.abs(Wm)).reshape(n, oh, ow, -1), kh * kw * cin_s

    def gemm(self, op, t, mut=None):
        mut = mut or {}
        W = op["W"]
        if mut.get("drop_granule_last_tap"):  # one 8-channel granule of the last tap of a k x k conv left out
            W = W.copy()
            W[:, 0:8, -1, -1] = 0.0
        if mut.get("drop_last_k_tile"):  # a linear's last K tile (64 stored channels, f16 build) left out
            W = W.copy()
            W[(-(-W.shape[0] // 64) - 1) * 64:] = 0.0
        acc, S, K = self._product(op, t[gi(op, "i")], W, wrap_pad=bool(mut.get("pad_tap_from_neighbour")))
        b = op["b"]
        if op["kind"] == "deconv":  # taps (dy, dx) to pixels (2y + dy, 2x + dx)
            n, h, w, _, co = acc.shape
            tp = (0, 1, 4, 2, 3, 5) if mut.get("deconv_swap_taps") else (0, 1, 3, 2, 4, 5)
            unt = lambda a: a.reshape(n, h, w, 2, 2, co).transpose(*tp).reshape(n, 2 * h, 2 * w, co)
            acc, S = unt(acc), unt(S)
        s_, t_ = op["s"], op["t"]
        if s_ is not None:  # (f32 twin: the oracle's bias | scale | shift, here folded in f64)
            acc, S = acc * s_, S * np.abs(s_)
            b = (b * s_ if b is not None else 0.0) + t_
        bb = np.zeros(acc.shape[-1]) if b is None else b.copy()
        if mut.get("drop_last_bias"):
            bb[-1] = 0.0
        pre = acc + bb
        ra = 0.0
        if op["res"] is not None:
            rt, up = op["res"]
            r = t[rt]
            if up > 1:
                if mut.get("addup_shift_x"):  # the residual taken at (y / 2, x / 2 + 1) (the last column: its own)
                    r = r[:, :, np.minimum(np.arange(r.shape[2]) + 1, r.shape[2] - 1)]
                r = np.repeat(np.repeat(r, up, 1), up, 2)
            if mut.get("drop_res_last_row"):
                r = r.copy()
                r.reshape(-1, r.shape[-1])[-1] = 0.0
            pre = pre + r
            ra = np.abs(r)
        y, aerr = _act(op["act"], pre, self.half)
        if mut.get("last_row_from_previous") and y.reshape(-1, y.shape[-1]).shape[0] > 1:  # the last row of the last (partial) M tile
            y = y.copy()
            y.reshape(-1, y.shape[-1])[-1] = y.reshape(-1, y.shape[-1])[-2]
        if mut.get("drop_last_column"):  # the last existing column written as a pad channel
            y = y.copy()
            y[..., -1] = 0.0
        f32_out = gi(op, "o") == self.out_tid
        ep = 2 * U32 * (np.abs(bb) + ra) if self.half else 4 * U32 * (np.abs(acc) + np.abs(bb) + ra)
        bound = ACT_L[op["act"]] * (K * U32 * S + ep) + aerr + self._out_round(y, f32_out)
        return (y if f32_out or not self.half else np.clip(y, -F16_MAX, F16_MAX)), bound

    def deconv_map(self, op, x, w4_f16=False):
        """2x2 stride-2 transposed conv to one channel + bias + sigmoid: the f32 probability map [N, 2H, 2W, 1]"""
        W = np.asarray(self.P[op["kv"]["w"]], np.float32).astype(np.float64)[:, 0]  # [ci][2][2]
        if w4_f16:
            W = f16(W)
        b = [float(np.float32(self.P[a[0]][0])) for k, a in op["ep"] if k == "bias"][0]
        n, h, w, c = x.shape
        A = x.reshape(-1, c)
        acc = (A @ W.reshape(c, 4)).reshape(n, h, w, 2, 2)
        S = (np.abs(A) @ np.abs(W.reshape(c, 4))).reshape(n, h, w, 2, 2)
        y, aerr = _act("sigmoid", acc + b, False)
        bound = 0.25 * (c * U32 * S + 2 * U32 * abs(b)) + aerr + 4 * U32
        unt = lambda a: a.transpose(0, 1, 3, 2, 4).reshape(n, 2 * h, 2 * w, 1)
        return unt(y), unt(bound)

    def pool(self, op, x, mut=None):
        kh, kw, sh, sw, ph, pw = (gi(op, q) for q in ("kh", "kw", "sh", "sw", "ph", "pw"))
        n, h, w, c = x.shape
        oh, ow = (h + 2 * ph - kh) // sh + 1, (w + 2 * pw - kw) // sw + 1
        mx = op["kv"]["type"] == "max"
        xp = np.pad(x, ((0, 0), (ph, ph), (pw, pw), (0, 0)), constant_values=-np.inf if mx else 0.0)
        ones = np.pad(np.ones((1, h, w, 1)), ((0, 0), (ph, ph), (pw, pw), (0, 0)))
        acc = np.full((n, oh, ow, c), -np.inf) if mx else np.zeros((n, oh, ow, c))
        cnt, sab = np.zeros((1, oh, ow, 1)), np.zeros((n, oh, ow, c))
        for y in range(kh):
            for xx in range(kw):
                win = xp[:, y:y + sh * (oh - 1) + 1:sh, xx:xx + sw * (ow - 1) + 1:sw]
                if mx:
                    acc = np.maximum(acc, win)
                else:
                    acc = acc + win
                    sab = sab + np.abs(win)
                cnt = cnt + ones[:, y:y + sh * (oh - 1) + 1:sh, xx:xx + sw * (ow - 1) + 1:sw]
        if mx:
            return acc, None
        if (mut or {}).get("avg_include_pad"):
            cnt = np.full_like(cnt, kh * kw)
        y = acc / cnt
        return y, (kh * kw) * U32 * sab / cnt + 2 * U32 * np.abs(y) + self._out_round(y)

    def addpos(self, op, x):
        n, h, w, c = x.shape
        pos = np.asarray(self.P[op["ep"][0][1][0]], np.float32).astype(np.float64).reshape(1, h, w, c)
        y = x + pos
        return y, U32 * np.abs(y) + self._out_round(y)

    @staticmethod
    def ln_stats(x, eps, pivot=False, unbiased=False):
        """(m, r, dm, dr): mean, rstd and the bounds of their f32 errors (two passes; pivot: one pass shifted by the first channel)"""
        C = x.shape[-1]
        m = x.mean(-1, keepdims=True)
        var = ((x - m) ** 2).sum(-1, keepdims=True) / (C - 1 if unbiased else C)
        r = 1.0 / np.sqrt(var + eps)
        dm = C * U32 * np.abs(x).sum(-1, keepdims=True) / C + U32 * np.abs(m)
        grow = 1.0 + ((m - x[..., :1]) ** 2 / np.maximum(var, 1e-300) if pivot else 0.0)
        vrel = (C + 3) * U32 * grow + dm ** 2 / np.maximum(var, 1e-300)
        dr = 0.5 * np.minimum(vrel * var / (var + eps), 1.0) + 2 * U32
        return m, r, dm, dr

    def ln(self, op, x, mut=None):
        g = np.asarray(self.P[op["kv"]["g"]], np.float32).astype(np.float64)
        b = np.asarray(self.P[op["kv"]["b"]], np.float32).astype(np.float64)
        m, r, dm, dr = self.ln_stats(x, float(op["kv"]["eps"]), unbiased=(mut or {}).get("ln_unbiased", False))
        z = (x - m) * r
        y = z * g + b
        bound = np.abs(g) * r * (dm + np.abs(x - m) * (dr + 4 * U32)) + 2 * U32 * np.abs(b) + self._out_round(y)
        return y, bound

    def attn(self, op, x, mut=None):
        heads, hd, gh, gw, lh, lw = (gi(op, q) for q in ("heads", "hd", "gh", "gw", "lh", "lw"))
        scale = float(np.float32(op["kv"]["scale"]))
        n, h, w, c3 = x.shape
        T, D = h * w, heads * hd
        qkv = x.reshape(n, T, 3, heads, hd).transpose(2, 0, 3, 1, 4)  # [3][n][heads][T][hd]
        q, k, v = qkv
        if self.half:  # q scale log2(e) rounded to f16 (the kernel's Q fragments); logits in base 2
            q = f16((q.astype(np.float32) * np.float32(scale * LOG2E)).astype(np.float64))
            base = 2.0
        else:
            q = q * scale
            base = math.e
        S = q @ k.transpose(0, 1, 3, 2)
        Sa = np.abs(q) @ np.abs(k.transpose(0, 1, 3, 2))
        yy, xx = np.divmod(np.arange(T), w)
        ok = np.ones((T, T), bool)
        if lh > 0:
            ok = (np.abs(yy[:, None] - yy[None]) <= lh // 2) & (np.abs(xx[:, None] - xx[None]) <= lw // 2)
            if (mut or {}).get("window_shift_right_border"):  # queries whose window meets the right border see one column further left
                qx = xx[:, None]
                edge = qx + lw // 2 >= w
                d = xx[None] - qx
                shifted = (np.abs(yy[:, None] - yy[None]) <= lh // 2) & (d >= -(lw // 2) - 1) & (d <= lw // 2 - 1)
                ok = np.where(edge, shifted, ok)
        S = np.where(ok, S, -np.inf)
        mrow = S.max(-1, keepdims=True)
        p = np.power(base, S - mrow)
        l = p.sum(-1, keepdims=True)
        P = p / l
        o = P @ v
        nk = ok.sum(-1)[None, None, :, None]
        # per key: logit error (f32 sum over hd, the subtraction of m) -> relative error of p; its maximum over the row's keys
        e = U32 * (hd * Sa + np.abs(np.where(ok, S, 0.0)) + np.abs(mrow))
        eps_ = np.where(ok, (LN2 if self.half else 1.0) * e, 0.0).max(-1, keepdims=True) + 2.0 ** -22
        up = U16 if self.half else 0.0
        Pv = P @ np.abs(v)
        bound = (2.02 * eps_ + up + (nk + 4) * U32) * Pv + (SUB if self.half else 0.0) * (ok.astype(np.float64) @ np.abs(v)) / l
        y = o.transpose(0, 2, 1, 3).reshape(n, h, w, D)
        bound = bound.transpose(0, 2, 1, 3).reshape(n, h, w, D) + self._out_round(y)
        return y, bound

    # ----------------------------------------------------------------------------------------------------------- fused launches
    def mlp(self, f1, f2, u, absorbed=None):
        """SVTR's MLP as srv_mlp.h runs it: y = res + fc2(f16(gelu(fc1))) + b2; absorbed = the `ln` op in front (its LayerNorm
        inside: fc1 = r (u W1') - r m s + c, res = LN(u) in f32).  u: the launch's input [.., C] as the device holds it"""
        C = u.shape[-1]
        A = u.reshape(-1, C)
        W2, b2 = f2["W"], f2["b"]
        if absorbed is None:
            W1, b1 = f1["W"], f1["b"]
            pre = A @ W1 + b1
            b_pre = C * U32 * (np.abs(A) @ np.abs(W1)) + 2 * U32 * np.abs(b1)
            res, b_res = A, 0.0
        else:
            F = self.ln_fold[next(k for k, o in enumerate(self.ops) if o is f1)]
            m, r, dm, dr = self.ln_stats(A, F["eps"], pivot=True)
            acc = A @ F["W1"]
            pre = r * (acc - m * F["s"]) + F["c"]
            # the f32 sum of u W1' (on u, not u - m), r and m with their errors, the two f32 fmas
            b_pre = (r * (C * U32 * (np.abs(A) @ np.abs(F["W1"])) + dm * np.abs(F["s"]) + 2 * U32 * np.abs(m * F["s"]))
                     + np.abs(pre - F["c"]) * (dr + 2 * U32) + 2 * U32 * np.abs(F["c"]))
            res = (A - m) * r * F["g"] + F["b"]
            b_res = np.abs(F["g"]) * r * (dm + np.abs(A - m) * (dr + 4 * U32)) + 2 * U32 * np.abs(F["b"])
        h, herr = _act("gelu", pre, True)
        b_h = ACT_L["gelu"] * b_pre + herr + U16 * np.abs(h) + SUB
        y = res + h @ W2 + b2
        b_y = (b_h @ np.abs(W2) + 4 * C * U32 * (np.abs(h) @ np.abs(W2)) + b_res + 2 * U32 * (np.abs(b2) + np.abs(res))
               + U16 * np.abs(y) + SUB)
        shp = u.shape[:-1] + (C,)
        return np.clip(y, -F16_MAX, F16_MAX).reshape(shp), b_y.reshape(shp)

    def head_tail(self, d1, d2, x):
        """head_tail_kernel: mid = relu(deconv 64 -> 64 + b) rounded to f16 (kept in f64 here, its rounding in the bound), then the
        second transposed conv on f16 weights on the matrix pipe, + bias, sigmoid -> the f32 map [N, 4H, 4W, 1]"""
        mid, b_mid = self.gemm(dict(d1, res=None), {gi(d1, "i"): x})
        b_mid = b_mid  # (gemm's bound holds the f16 rounding of mid)
        W = f16(np.asarray(self.P[d2["kv"]["w"]], np.float32).astype(np.float64)[:, 0]).reshape(-1, 4)
        b = [float(np.float32(self.P[a[0]][0])) for k, a in d2["ep"] if k == "bias"][0]
        n, h, w, c = mid.shape
        A = mid.reshape(-1, c)
        acc = A @ W + b
        S = np.abs(A) @ np.abs(W)
        prop = b_mid.reshape(-1, c) @ np.abs(W)
        y, aerr = _act("sigmoid", acc, False)
        bound = 0.25 * (prop + c * U32 * S + 2 * U32 * abs(b)) + aerr + 2.0 ** -21
        unt = lambda a: a.reshape(n, h, w, 2, 2).transpose(0, 1, 3, 2, 4).reshape(n, 2 * h, 2 * w, 1)
        return unt(y), unt(bound)


def ratio(got, ref, bound):
    """max over elements of |got - ref| / bound (inf where got is not finite; exact ops: 0 if equal, else inf)"""
    got = np.asarray(got, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if not np.isfinite(got).all():
        return math.inf
    if bound is None:
        return 0.0 if np.array_equal(got, ref) else math.inf
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    return float(r.max()) if got.size else 0.0


def kind_of(op, launch_name=""):
    """the op kind a worst-ratio line is reported under"""
    k = op["kind"]
    if k == "conv":
        return "conv%sx%s" % (gi(op, "kh"), gi(op, "kw"))
    if k == "linear":
        return "linear_" + op.get("act", "none") + ("_res" if op.get("res") else "")
    if k == "deconv":
        return "deconv_map" if gi(op, "cout") == 1 else "deconv"
    if k == "pool":
        return "pool_" + op["kv"]["type"]
    if k == "attn":
        return "attn_" + ("local" if gi(op, "lh") > 0 else "global")
    return {"ew": "addpos"}.get(k, k)


# the six errors the checker must reject (each local or small: what whole-network tolerances do not see)
MUTATIONS = ("drop_res_last_row", "drop_last_bias", "window_shift_right_border", "drop_granule_last_tap", "ln_unbiased", "avg_include_pad")


# seven errors of a tile edge or an index of the GEMM family (tests/srv_gemm_cases.py has an op for each; MUTATIONS above stays as it is)
GEMM_MUTATIONS = ("last_row_from_previous", "drop_last_column", "drop_last_k_tile", "pad_tap_from_neighbour", "deconv_swap_taps", "addup_shift_x",
                  "concat_next_shift")


def gemm_mutation_sites(ref, mut):
    """the ops of the plan a GEMM mutation changes (concat_next_shift: the concat ops - the conv behind one is then checked on the
    mutated concatenation)"""
    out = []
    for op in ref.ops:
        k = op["kind"]
        gemm = k in ("conv", "linear") or (k == "deconv" and gi(op, "cout") > 1)
        if ((mut in ("last_row_from_previous", "drop_last_column") and gemm and k != "deconv")
                or (mut == "drop_last_k_tile" and k == "linear" and op["W"].shape[0] > 64)
                or (mut == "pad_tap_from_neighbour" and k == "conv" and (gi(op, "ph") or gi(op, "pw")))
                or (mut == "deconv_swap_taps" and k == "deconv" and gi(op, "cout") > 1)
                or (mut == "addup_shift_x" and gemm and op["res"] is not None and op["res"][1] == 2)
                or (mut == "concat_next_shift" and k == "concat" and len(op["ins"]) > 1)):
            out.append(op)
    return out


# --------------------------------------------------------------------------------------------------------------- whole plan, torch
def torch_run(plan_text, params, x):
    """float64 torch interpretation of a server plan, op by op, written from the plan grammar alone"""
    import torch
    import torch.nn.functional as F
    t = {0: torch.from_numpy(x.astype(np.float64)).permute(0, 3, 1, 2)}
    P = {k: torch.from_numpy(np.asarray(v, np.float64)) for k, v in params.items()}

    def ep(y, stages):
        for st in stages:
            k, _, a = st.partition(":")
            a = a.split(",")
            if k == "bias":
                y = y + P[a[0]].view(1, -1, 1, 1)
            elif k == "bn":
                g, b, m, v = (P[n] for n in a[:4])
                y = (y - m.view(1, -1, 1, 1)) / torch.sqrt(v.view(1, -1, 1, 1) + float(a[4])) * g.view(1, -1, 1, 1) + b.view(1, -1, 1, 1)
            elif k == "addt":
                y = y + t[int(a[0])]
            elif k == "addup":
                y = y + F.interpolate(t[int(a[0])], scale_factor=int(a[1]), mode="nearest")
            elif k == "addpos":
                n, c, h, w = y.shape
                y = y + P[a[0]].view(1, h, w, c).permute(0, 3, 1, 2)
            elif k == "act":
                y = {"relu": F.relu, "gelu": lambda z: F.gelu(z), "hswish": F.hardswish, "sigmoid": torch.sigmoid}[a[0]](y)
            else:
                raise ValueError(k)
        return y

    out = None
    for line in plan_text.splitlines():
        if not line or line[0] == "#" or line.startswith("plan "):
            continue
        toks = line.split()
        kind, kv = toks[0], dict(tk.split("=", 1) for tk in toks[1:])
        stages = kv.get("ep", "").split("|") if kv.get("ep") else []
        gi_ = lambda k, d=0: int(kv.get(k, d))
        if kind == "output":
            out = t[gi_("i")]
            continue
        o = gi_("o")
        if kind == "conv":
            y = F.conv2d(t[gi_("i")], P[kv["w"]], stride=(gi_("sh"), gi_("sw")), padding=(gi_("ph"), gi_("pw")))
        elif kind == "linear":
            y = torch.einsum("nchw,co->nohw", t[gi_("i")], P[kv["w"]])
        elif kind == "deconv":
            y = F.conv_transpose2d(t[gi_("i")], P[kv["w"]], stride=2)
        elif kind == "pool":
            a = dict(kernel_size=(gi_("kh"), gi_("kw")), stride=(gi_("sh"), gi_("sw")), padding=(gi_("ph"), gi_("pw")))
            y = F.max_pool2d(t[gi_("i")], **a) if kv["type"] == "max" else F.avg_pool2d(t[gi_("i")], count_include_pad=False, **a)
        elif kind == "concat":
            ids, ups = [int(v) for v in kv["i"].split(",")], [int(v) for v in kv["up"].split(",")]
            y = torch.cat([F.interpolate(t[i], scale_factor=u, mode="nearest") if u > 1 else t[i] for i, u in zip(ids, ups)], 1)
        elif kind == "ew":
            y = t[gi_("i")]
        elif kind == "ln":
            z = t[gi_("i")].permute(0, 2, 3, 1)
            y = F.layer_norm(z, z.shape[-1:], P[kv["g"]], P[kv["b"]], float(kv["eps"])).permute(0, 3, 1, 2)
        elif kind == "attn":
            z = t[gi_("i")]
            n, c3, h, w = z.shape
            heads, hd = gi_("heads"), gi_("hd")
            T = h * w
            q, k, v = z.permute(0, 2, 3, 1).reshape(n, T, 3, heads, hd).permute(2, 0, 3, 1, 4)
            s = (q * float(kv["scale"])) @ k.transpose(-1, -2)
            lh, lw = gi_("lh"), gi_("lw")
            if lh > 0:  # SVTR's Local mixer: -inf outside the window (rec_svtrnet.py builds this mask by slicing a padded grid)
                yy, xx = np.divmod(np.arange(T), w)
                ok = (np.abs(yy[:, None] - yy[None]) <= lh // 2) & (np.abs(xx[:, None] - xx[None]) <= lw // 2)
                s = s.masked_fill(~torch.from_numpy(ok), float("-inf"))
            y = (torch.softmax(s, -1) @ v).permute(0, 2, 1, 3).reshape(n, h, w, heads * hd).permute(0, 3, 1, 2)
        else:
            raise ValueError(kind)
        t[o] = ep(y, stages)
    return out.permute(0, 2, 3, 1).numpy(), {k: v.permute(0, 2, 3, 1).numpy() for k, v in t.items() if k}


# --------------------------------------------------------------------------------------------------------------- checking a run
def mutation_site(ref, mut):
    """the op of the plan a mutation is applied to (None: the plan has no op it changes)"""
    for op in ref.ops:
        k = op["kind"]
        if mut == "drop_res_last_row" and k == "linear" and op["res"] is not None:
            return op
        if mut == "drop_last_bias" and k == "linear" and op["b"] is not None and abs(op["b"][-1]) >= 0.02:
            return op
        if mut == "window_shift_right_border" and k == "attn" and gi(op, "lh") > 0:
            return op
        if mut == "drop_granule_last_tap" and k == "conv" and gi(op, "kh") == 3 and gi(op, "cin") % 64 == 0:
            return op
        if mut == "ln_unbiased" and k == "ln":
            return op
        if mut == "avg_include_pad" and k == "pool" and op["kv"]["type"] == "avg" and (gi(op, "ph") or gi(op, "pw")):
            return op
    return None


def check_tensors(ref, t):
    """every op of the plan on the tensors t of one run (tid -> f64 NHWC, t[0] = the packed input as the device holds it):
    {op index: (kind, max err / bound)}"""
    res = {}
    for k, op in enumerate(ref.ops):
        if op["kind"] == "output":
            continue
        y, bound = ref.op(op, t)
        res[k] = (kind_of(op), ratio(t[gi(op, "o")], y, bound))
    return res


# ---------------------------------------------------------------------------------------------------------------- CTC tail
def ctc_tail(x, kind):
    """x f64 [rows, C] logits (finite maximum per row) -> (first maximum, p = 1 / sum exp(x - M), its bound); kind "two_pass" |
    "one_pass" (module docstring)"""
    x = np.asarray(x, dtype=np.float64)
    C = x.shape[-1]
    M = x.max(-1, keepdims=True)
    d = np.where(np.isfinite(x), np.abs(x - M), 0.0).max(-1)
    p = 1.0 / np.exp(x - M).sum(-1)
    if kind == "two_pass":
        rel = U32 * d + 4 * U32 + (-(-C // 64) + 6) * U32 + 2 * U32
    else:
        assert kind == "one_pass"
        rel = 3 * U32 * d + 9 * U32 * -(-C // 256) + 36 * U32 + 2 * U32
    return x.argmax(-1), p, p * rel * (1.0 + 2.0 ** -10)


def ctc_fold(m, s):
    """per-slot partials m, s f64 [rows, slots] (maximum, sum of exp(x - maximum)) of the slots that are folded -> (p, its bound)"""
    m, s = np.asarray(m, dtype=np.float64), np.asarray(s, dtype=np.float64)
    M = m.max(-1, keepdims=True)
    live = np.isfinite(m)
    p = 1.0 / np.where(live, s * np.exp(np.where(live, m - M, 0.0)), 0.0).sum(-1)
    d = np.where(live, np.abs(m - M), 0.0).max(-1)
    rel = 3 * U32 * d + 6 * U32 * m.shape[-1] + 2 * U32
    return p, p * rel * (1.0 + 2.0 ** -10)


def ctc_head(y, slots, step):
    """y f64 [rows, C] exact logits of a head run in partial mode, its slot count and step -> (first maximum, p, its bound)"""
    y = np.asarray(y, dtype=np.float64)
    M = y.max(-1, keepdims=True)
    d = np.abs(y - M).max(-1)
    p = 1.0 / np.exp(y - M).sum(-1)
    rel = 3 * U32 * d + 4 * U32 + 64 * step * U32 + 36 * U32 + 6 * U32 * -(-slots // step) + 2 * U32
    return y.argmax(-1), p, p * rel * (1.0 + 2.0 ** -10)


def linear_f32_bound(A, W, b, y):
    """the GEMM bound of the module docstring for an f32-output linear without activation: K u32 S + 2 u32 |b| + u32 |y|"""
    return A.shape[1] * U32 * (np.abs(A) @ np.abs(W)) + 2 * U32 * np.abs(b) + U32 * np.abs(y)
