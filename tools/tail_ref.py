"""Plain numpy restatement of the recognizer's tail: what turns a row of logits into (arg max, probability) and a line's steps into
characters (csrc/kernels_net.hip softmax_argmax_kernel / head_combine_kernel, csrc/srv_kernels.hip argmax_softmax*_kernel /
ctc_reduce_kernel, csrc/kernels_pre.hip ctc_kernel / ctc_chars_kernel).  In the spirit of pre_ref.py: written from the rules, proved
against the oracle library on the CPU (tests/test_tail_ref.py), then the yardstick of the device (tests/test_gpu_rec_tail.py), which
lets those tests carry its mutations.

The rules:
  row softmax, canonical order: columns in groups of 128; per group its maximum m_g (fmaxf: a NaN is skipped) and s_g = chain0 +
    chain1, chain h = the columns with ((c >> 2) & 1) == h, each summed in ascending column order of ocr_expf(x_c - m_g); per row
    M = max_g m_g, S = sum over ascending g of s_g * ocr_expf(m_g - M); p_c = ocr_expf(x_c - M) / S.  ocr_expf clamps its argument
    into [-87, 88] with fmaxf / fminf, so a NaN argument counts as -87.
  arg max: the first maximum of the LOGITS under `x > best` from best = -inf - a NaN is never the maximum; its probability is
    ocr_expf(x_best - M) / S.  A row in which no column exceeds -inf (all -inf and / or NaN) has none: (0, 0) is stored, column 0
    being the blank.  A probability that came out infinite (S underflowed to 0) is stored as 0.
  server fold: per 64-column slot (maximum, sum of exp(x - maximum), column of its first maximum); slots folded in ascending order,
    equal maxima keep the lower column; p = 1 / sum.  float64 here: the device is held to a derived bound (srv_ref.ctc_tail).
  greedy collapse: step n is kept iff amax[n] > 0 and (n == 0 or amax[n] != amax[n - 1]); the score is the f32 sum of the kept
    pmax[n] in step order divided by the count; ids are stored up to max_len, the count and the score's divisor are the FULL
    count.  With per-character evidence: the kept step, pmax there, and the length of the run of equal arg maxes from that step on
    (the run of the last stored character is closed when the next - cut - character starts, or at the line's end).

MUTATIONS: each switches ONE rule wrong; EQUIVALENT names those that cannot change any result, with the arithmetic."""
import numpy as np

MUTATIONS = ("last_maximum", "tie_to_later_group", "drop_partial_group", "collapse_across_blank", "score_over_stored", "open_last_run")
# last_maximum:          of equal maxima the last one wins
# tie_to_later_group:    inside a group (mobile: 128 columns; server: a 64-column slot) the first maximum wins, between groups the later
# drop_partial_group:    the last group / slot is left out when C is no multiple of its width
# collapse_across_blank: a repeat is dropped although a blank separates it from its twin (compared with the last NON-BLANK arg max)
# score_over_stored:     the score is divided by min(count, max_len)
# open_last_run:         the slot of the last stored character is not closed when a cut character starts: the run length of the
#                        line's last character is written into it
EQUIVALENT = {}

FILL = 0xA5       # OCR_SELFTEST_FILL
NO_MAX = 0x7fffffff
F32 = np.float32


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def filled(shape, dtype):
    """array whose every byte is FILL"""
    return np.full(tuple(shape) + (4,), FILL, np.uint8).view(dtype).reshape(shape)


# ------------------------------------------------------------------------------------------------------------ ocr_expf
def _fma(a, b, c):
    """fmaf on float32 arrays, exactly rounded: the product is exact in float64, the sum is rounded to odd there (TwoSum gives
    its error), and 53 >= 2 * 24 + 2 bits make the final rounding to float32 the single rounding of the exact value"""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    t = p + c
    bb = t - p
    err = (p - (t - bb)) + (c - bb)
    ti = t.view(np.int64).copy()
    need = (err != 0) & ((ti & 1) == 0)
    step = np.where((t > 0) == (err > 0), 1, -1)
    ti = np.where(need, ti + step, ti)
    return ti.view(np.float64).astype(F32)


def expf(x):
    """ocr_expf (csrc/ocr_common.h) on a float32 array: Cephes expf with a fixed sequence of f32 roundings"""
    x = np.asarray(x, dtype=F32)
    with np.errstate(invalid="ignore"):
        x = np.fmin(np.fmax(x, F32(-87.0)), F32(88.0))
    n = np.rint(x * F32(1.44269504088896341))
    r = _fma(n, np.full_like(x, F32(-0.693359375)), x)
    r = _fma(n, np.full_like(x, F32(2.12194440e-4)), r)
    p = np.full_like(x, F32(1.9875691500E-4))
    for k in (1.3981999507E-3, 8.3334519073E-3, 4.1665795894E-2, 1.6666665459E-1, 5.0000001201E-1):
        p = _fma(p, r, np.full_like(x, F32(k)))
    y = _fma(p, r * r, r) + F32(1.0)
    sc = ((n.astype(np.int32) + 127).astype(np.uint32) << np.uint32(23)).view(F32)
    return y * sc


# ------------------------------------------------------------------------------------------------------------ arg max
def first_maximum(x, mut=(), group=128):
    """[rows, C] -> (int32 [rows] column of the first maximum under `x > best` from -inf, NO_MAX where no column exceeds -inf,
    the value there (-inf where none))"""
    x = np.asarray(x)
    rows, C = x.shape
    if "drop_partial_group" in mut and C % group and C > group:
        x, C = x[:, :C - C % group], C - C % group
    v = np.where(np.isnan(x), -np.inf, x)
    best = v.max(1)
    hit = v == best[:, None]
    if "last_maximum" in mut:
        idx = C - 1 - hit[:, ::-1].argmax(1)
    elif "tie_to_later_group" in mut:
        g = (np.arange(C) // group)[None, :]
        last_g = np.where(hit, g, -1).max(1)
        idx = (hit & (g == last_g[:, None])).argmax(1)
    else:
        idx = hit.argmax(1)
    none = ~(best > -np.inf)
    return np.where(none, NO_MAX, idx).astype(np.int32), best


def _finish(idx, p):
    """head_result (csrc/ocr_common.h): no maximum -> (0, 0); an infinite probability -> 0"""
    none = idx == NO_MAX
    p = np.where(none | np.isinf(p), F32(0), p).astype(F32)
    return np.where(none, 0, idx).astype(np.int32), p


# ------------------------------------------------------------------------------------------------------ mobile heads, f32
def group_partials(x, mut=()):
    """f32 [rows, C] -> (m [rows, G], s [rows, G] f32, idx [rows, G] int32): per group of 128 columns its maximum, chain0 + chain1 of
    ocr_expf(x - m) and the column of its first maximum (NO_MAX: none) - what conv_finish<OUT_HEAD> hands to head_combine_kernel"""
    x = np.asarray(x, dtype=F32)
    rows, C = x.shape
    G = (C + 127) // 128
    if "drop_partial_group" in mut and C % 128 and G > 1:
        G -= 1
    pad = np.full((rows, G * 128), np.nan, F32)
    pad[:, :min(C, G * 128)] = x[:, :G * 128]
    pad = pad.reshape(rows, G, 128)
    valid = (np.arange(G * 128) < C).reshape(1, G, 128)
    with np.errstate(invalid="ignore"):
        m = np.fmax.reduce(np.where(valid, pad, F32(-np.inf)), axis=2, initial=F32(-np.inf)).astype(F32)
        e = expf(pad - m[:, :, None])
    ch = np.zeros((rows, G, 2), F32)
    for c in range(128):
        h = (c >> 2) & 1
        ch[:, :, h] = np.where(valid[:, :, c], ch[:, :, h] + e[:, :, c], ch[:, :, h])
    idx = np.empty((rows, G), np.int32)
    for g in range(G):
        i, _ = first_maximum(x[:, g * 128:min(C, g * 128 + 128)], mut=tuple(k for k in mut if k == "last_maximum"))
        idx[:, g] = np.where(i == NO_MAX, NO_MAX, i + g * 128)
    return m, (ch[:, :, 0] + ch[:, :, 1]).astype(F32), idx


def combine(m, s, idx, mut=()):
    """head_combine_kernel's rule on group partials -> (amax int32 [rows], pmax f32 [rows], M, S)"""
    m, s = np.asarray(m, dtype=F32), np.asarray(s, dtype=F32)
    rows, G = m.shape
    with np.errstate(invalid="ignore"):
        M = np.fmax.reduce(m, axis=1, initial=F32(-np.inf)).astype(F32)
        S = np.zeros(rows, F32)
        for g in range(G):
            S = S + s[:, g] * expf(m[:, g] - M)
        v = np.where(np.isnan(m), -np.inf, m)
        hit = (v == M[:, None]) & (M[:, None] > -np.inf)
        later = "tie_to_later_group" in mut or "last_maximum" in mut
        g_win = (G - 1 - hit[:, ::-1].argmax(1)) if later else hit.argmax(1)
        amax = np.where(hit.any(1), np.asarray(idx)[np.arange(rows), g_win], NO_MAX).astype(np.int32)
        with np.errstate(divide="ignore"):
            p = expf(M - M) / S
    amax, p = _finish(amax, p)
    return amax, p, M, S


def softmax32(x, mut=(), probs=False):
    """the canonical f32 row softmax + arg max (softmax_argmax_kernel; == group_partials + combine) -> (amax, pmax[, probs])"""
    x = np.asarray(x, dtype=F32)
    m, s, idx = group_partials(x, mut)
    amax, pmax, M, S = combine(m, s, idx, mut)
    if not probs:
        return amax, pmax
    with np.errstate(invalid="ignore", divide="ignore"):
        q = expf(x - M[:, None]) / S[:, None]
    return amax, pmax, q.astype(F32)


def softmax64(x, mut=()):
    """float64: (first maximum, exp(x_best - M) / sum exp(x - M)) of rows with a finite maximum"""
    x = np.asarray(x, dtype=np.float64)
    idx, best = first_maximum(x, mut)
    if "drop_partial_group" in mut and x.shape[1] % 128 and x.shape[1] > 128:
        x = x[:, :x.shape[1] - x.shape[1] % 128]
    return idx, 1.0 / np.exp(x - best[:, None]).sum(1)


# ------------------------------------------------------------------------------------------------------ server fold, f64
def srv_partials(x, mut=()):
    """[rows, C] -> f64 m, s [rows, slots] and int32 idx [rows, slots]: per 64-column slot (maximum, sum of exp(x - maximum), column
    of its first maximum) - what the head's matrix kernel leaves per row (GemmArgs::ctc_part)"""
    x = np.asarray(x, dtype=np.float64)
    rows, C = x.shape
    slots = (C + 63) // 64
    if "drop_partial_group" in mut and C % 64 and slots > 1:
        slots -= 1
    m, s, idx = np.empty((rows, slots)), np.empty((rows, slots)), np.empty((rows, slots), np.int32)
    for k in range(slots):
        blk = x[:, k * 64:min(C, k * 64 + 64)]
        i, b = first_maximum(blk, mut=tuple(q for q in mut if q == "last_maximum"))
        m[:, k] = b
        with np.errstate(invalid="ignore"):
            s[:, k] = np.where(b > -np.inf, np.exp(blk - b[:, None]).sum(1), 0.0)
        idx[:, k] = np.where(i == NO_MAX, NO_MAX, i + k * 64)
    return m, s, idx


def pack_partials(m, s, idx):
    """f32 [rows, slots, 4] as ctc_reduce_kernel reads them (the column as int bits)"""
    out = np.zeros(m.shape + (4,), F32)
    out[..., 0], out[..., 1] = m, s
    out[..., 2] = np.asarray(idx, dtype=np.int32).view(F32)
    return out


def srv_fold(m, s, idx, step=1, mut=()):
    """slots 0, step, 2 step, .. folded: equal maxima keep the lower COLUMN -> (amax int32, p f64 = 1 / sum; (0, 0) without a maximum)"""
    m, s, idx = (np.asarray(a)[:, ::step] for a in (m, s, idx))
    rows = m.shape[0]
    v = np.where(np.isnan(m), -np.inf, m)
    M = v.max(1)
    hit = (v == M[:, None]) & (M[:, None] > -np.inf)
    if "tie_to_later_group" in mut or "last_maximum" in mut:
        amax = np.where(hit, idx, -1).max(1)
    else:
        amax = np.where(hit, idx, NO_MAX).min(1)
    amax = np.where(hit.any(1), amax, NO_MAX)
    with np.errstate(invalid="ignore", divide="ignore"):
        tot = np.where(v > -np.inf, s * np.exp(np.where(v > -np.inf, m - M[:, None], 0.0)), 0.0).sum(1)
        p = 1.0 / tot
    none = amax == NO_MAX
    return np.where(none, 0, amax).astype(np.int32), np.where(none | np.isinf(p), 0.0, p)


# ------------------------------------------------------------------------------------------------------------ collapse
def collapse(amax, pmax, mut=()):
    """greedy CTC collapse of ONE line that keeps where every character came from -> (ids, steps, nsteps, probs), uncut"""
    ids, steps, nsteps, probs = [], [], [], []
    last = 0
    for n, a in enumerate(amax):
        if a > 0 and not (n > 0 and a == last):
            ids.append(int(a)); steps.append(n); nsteps.append(1); probs.append(pmax[n])
        elif a > 0:
            nsteps[-1] += 1
        if not ("collapse_across_blank" in mut and a == 0 and n > 0):
            last = a
    return np.array(ids, np.int32), np.array(steps, np.int32), np.array(nsteps, np.int32), np.array(probs, np.float32)


def ctc(amax, pmax, lines, max_len, chars=False, mut=()):
    """lines: list of (first step, steps) into the flat step arrays -> dict: ids [n, max_len] (FILL past the stored count), lens
    [n] (the full count), scores [n] (sequential f32 sum / full count; 0 for an empty line) and, with chars, steps / nsteps / probs
    [n, max_len]"""
    amax, pmax = np.asarray(amax, dtype=np.int32).reshape(-1), np.asarray(pmax, dtype=F32).reshape(-1)
    n = len(lines)
    out = {"ids": filled((n, max_len), np.int32), "lens": np.zeros(n, np.int32), "scores": np.zeros(n, F32)}
    if chars:
        out.update(steps=filled((n, max_len), np.int32), nsteps=filled((n, max_len), np.int32), probs=filled((n, max_len), F32))
    for li, (s0, T) in enumerate(lines):
        am, pm = amax[s0:s0 + T], pmax[s0:s0 + T]
        ids, steps, nsteps, probs = collapse(am, pm, mut)
        cnt = len(ids)
        k = min(cnt, max_len)
        s = F32(0)
        for p in probs:
            s = F32(s + p)
        out["ids"][li, :k] = ids[:k]
        out["lens"][li] = cnt
        div = k if "score_over_stored" in mut else cnt
        out["scores"][li] = F32(s / F32(div)) if cnt > 0 else F32(0)
        if chars:
            if "open_last_run" in mut and cnt > max_len:  # the slot of the last stored character stays open: the line's last run lands in it
                nsteps = nsteps.copy()
                nsteps[k - 1] = nsteps[-1]
            out["steps"][li, :k], out["nsteps"][li, :k], out["probs"][li, :k] = steps[:k], nsteps[:k], probs[:k]
    return out
