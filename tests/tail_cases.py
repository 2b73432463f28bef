"""The case tables of the recognizer-tail tests: tests/test_tail_ref.py proves tools/tail_ref.py on them (and that every designed
branch occurs in them), tests/test_gpu_rec_tail.py runs the device on them.  Logits of the arg-max cases are small integers, so
ties are true ties and every value is exact in f32."""
import numpy as np

HEAD_C = (2, 127, 128, 129, 255, 257, 6625)
HEAD_ROWS = (1, 3, 4, 5, 255, 256, 257)   # the row quad of softmax_argmax_kernel / argmax_softmax*, the 256-thread blocks of the folds
ROWS_C = 129                              # the column count of the row-count cases
TOP, TIE_FLOOR = 9, 5                     # designed maxima hold TOP; every other logit is an integer in [-30, TIE_FLOOR]

# name -> columns that hold the row's maximum (the first of them must win); columns >= C drop out, an empty set drops the row
TIE_ROWS = (
    ("first", (0,)), ("last", (-1,)), ("group_end", (127,)), ("group_start", (128,)), ("tie_127_128", (127, 128)),
    ("tie_two_groups", (128, 5)), ("tie_last_group", (5, -1)), ("slot_end", (63,)), ("slot_start", (64,)), ("tie_63_64", (63, 64)),
    ("tie_two_slots", (70, 194)), ("tie_in_group", (10, 20)), ("tie_tiles_31_32", (31, 32)), ("tie_tiles_255_256", (255, 256)),
    ("tie_lanes", (1, 65)), ("all_equal", None),
)


def tie_rows(C, seed=0):
    """-> (names, f32 [n, C], int32 [n] designed arg max)"""
    rs = np.random.RandomState(1000 + 7 * C + seed)
    names, rows, want = [], [], []
    for name, cols in TIE_ROWS:
        if cols is None:
            names.append(name); rows.append(np.full(C, 3, np.float32)); want.append(0)
            continue
        cols = sorted({c if c >= 0 else C + c for c in cols if c < C})
        if len(cols) < (2 if name.startswith("tie") else 1):
            continue
        r = rs.randint(-30, TIE_FLOOR + 1, C).astype(np.float32)
        r[cols] = TOP
        names.append(name); rows.append(r); want.append(cols[0])
    return names, np.stack(rows), np.array(want, np.int32)


def head_cases():
    """name -> (f32 [rows, C], designed arg max): every C with its tie rows; every row count at C = ROWS_C, the tie rows cycled"""
    out = {}
    for C in HEAD_C:
        _, x, w = tie_rows(C)
        out["ties_C%d" % C] = (x, w)
    for R in HEAD_ROWS:
        xs, ws = [], []
        k = 0
        while sum(len(w) for w in ws) < R:
            _, x, w = tie_rows(ROWS_C, seed=100 + k)
            xs.append(x); ws.append(w); k += 1
        out["rows_%d" % R] = (np.concatenate(xs)[:R], np.concatenate(ws)[:R])
    return out


def random_rows(C, rows=9, scale=4.0):
    """real-valued rows for the probability checks (|x - max| stays far below ocr_expf's clamp at -87)"""
    return (np.random.RandomState(2000 + C).randn(rows, C) * scale).astype(np.float32)


DEGENERATE_C = (2, 129, 257)


def degenerate_rows(C):
    """-> (names, f32 [n, C]): rows without a finite maximum, and rows with one NaN"""
    rs = np.random.RandomState(3000 + C)
    base = lambda: rs.randint(-9, 6, C).astype(np.float32)
    names, rows = [], []

    def add(n, r):
        names.append(n); rows.append(r)
    add("all_neg_inf", np.full(C, -np.inf, np.float32))
    r = np.full(C, -np.inf, np.float32); r[C - 1] = 2.0; add("one_finite_last", r)
    r = np.full(C, -np.inf, np.float32); r[0] = -3.0; add("one_finite_first", r)
    r = base(); r[C // 2] = np.inf; add("pos_inf", r)
    r = base(); r[1] = np.inf; r[C - 1] = np.inf; add("two_pos_inf", r)
    add("all_nan", np.full(C, np.nan, np.float32))
    r = np.full(C, np.nan, np.float32); r[C - 1] = -np.inf; add("nan_and_neg_inf", r)
    r = base(); r[0] = np.nan; r[C - 1] = 7.0; add("nan_first", r)
    r = base(); r[C - 1] = np.nan; r[0] = 7.0; add("nan_last", r)
    r = base(); r[C // 2] = 7.0; r[C // 2 - 1] = np.nan; add("nan_before_max", r)
    add("plain", base() + np.float32(0.5))
    return names, np.stack(rows)


# ------------------------------------------------------------------------------------------------------------ collapse
MAX_LEN = 6
A, B = 7, 11


def _runs(count, total):
    """`count` characters alternating A, B with run lengths 1, 2, 3, 1, .. then blanks up to `total` steps"""
    out = []
    for j in range(count):
        out += [A if j % 2 == 0 else B] * (1 + j % 3)
    assert len(out) <= total
    return out + [0] * (total - len(out))


def designed_lines(T):
    """name -> arg maxes of one line of T steps (only those that fit)"""
    d = {"all_blank": [0] * T, "one_class": [A] * T, "char_at_0": [A] + [0] * (T - 1), "char_at_last": [0] * (T - 1) + [B]}
    if T >= 4:
        d["a_a_blank_a"] = [A, A, 0, A] + [0] * (T - 4)
        d["a_b_a"] = [A, B, A] + [0] * (T - 3)
        d["blank_first_repeat"] = [0, A, A, 0] + [B] * (T - 4)
    if T >= 40:
        for c in (MAX_LEN - 1, MAX_LEN, MAX_LEN + 1, 3 * MAX_LEN):
            d["count_%d" % c] = _runs(c, T)
        d["cut_then_runs"] = [A, B, A, B, A, B, B, B, B, A, A] + [0] * (T - 11)   # the last stored run (4) is closed; a cut run of 2 follows
        d["cut_no_repeat"] = [A, 0, B, 0, A, 0, B, 0, A, 0, B, B, 0, A] + [0] * (T - 14)
    return d


def _fill_lines(rs, lines, total, designed):
    amax = np.zeros(total, np.int32)
    pmax = (rs.rand(total) * 0.9 + 0.05).astype(np.float32)
    names = list(designed)
    for li, (s0, T) in enumerate(lines):
        if li < len(names) and len(designed[names[li]]) == T:
            amax[s0:s0 + T] = designed[names[li]]
        else:
            amax[s0:s0 + T] = rs.choice([0, 0, 0, 1, 1, 2, 3], T)
    return amax, pmax


def collapse_cases():
    """name -> dict(T (None: ragged), lines [(first step, steps)], amax, pmax, max_len, designed {line name -> line index})"""
    out = {}
    for n in (1, 63, 64, 65, 130):
        for T in (1, 2, 40):
            rs = np.random.RandomState(4000 + 100 * n + T)
            lines = [(i * T, T) for i in range(n)]
            d = designed_lines(T)
            amax, pmax = _fill_lines(rs, lines, n * T, d)
            out["n%d_T%d" % (n, T)] = dict(T=T, lines=lines, amax=amax, pmax=pmax, max_len=MAX_LEN,
                                           designed={k: i for i, k in enumerate(d) if i < n})
    c = dict(out["n65_T40"]); c["max_len"] = 1; out["n65_T40_maxlen1"] = c
    # ragged: steps 1, 2, 40, 83 mixed, the lines' first steps not in line order; the 40-step lines carry the designed ones
    rs = np.random.RandomState(4999)
    d = designed_lines(40)
    steps = [40] * len(d) + [(1, 2, 40, 83)[i % 4] for i in range(66 - len(d))]
    order = rs.permutation(len(steps))
    first = np.zeros(len(steps), np.int64)
    at = 3                                        # (the step arrays do not start with a line)
    for li in order:
        first[li] = at
        at += steps[li] + (li % 2)                # gaps no line owns
    lines = [(int(first[i]), steps[i]) for i in range(len(steps))]
    amax, pmax = _fill_lines(rs, lines, at + 5, d)
    out["ragged_66"] = dict(T=None, lines=lines, amax=amax, pmax=pmax, max_len=MAX_LEN, designed={k: i for i, k in enumerate(d)})
    return out


# ------------------------------------------------------------------------------------------------- server fused head, exact
SRV_K, SRV_C, SRV_BLOCK = 384, 6625, 32
# design -> columns that tie at the row's maximum (the first must win); one design per block of SRV_BLOCK input channels
SRV_DESIGNS = (
    ("first", (0,)), ("last", (6624,)), ("slot_end", (63,)), ("slot_start", (64,)), ("tie_63_64", (63, 64)), ("tie_two_slots", (70, 194)),
    ("tie_two_tiles", (5, 133, 261, 517)), ("tie_127_128", (127, 128)), ("tie_255_256", (255, 256)), ("tie_first_last", (5, 6624)),
    ("last_slot", (6591, 6592)), ("all_equal", None),
)


def srv_int_head():
    """small-integer weights [K, C] and bias [C] of a CTC head whose logits are exact in f32 in any summation order (|sum| < 2^24): in
    block k of the input channels the columns of design k carry weight 3, every other weight is in [-2, 2]; an input row that is
    non-negative and lives in block k alone therefore has its maximum exactly at the design's columns, all equal"""
    rs = np.random.RandomState(6000)
    W = rs.randint(-2, 3, (SRV_K, SRV_C)).astype(np.float32)
    b = (rs.rand(SRV_C) < 0.5).astype(np.float32)
    b[0] = 1
    for k, (_, cols) in enumerate(SRV_DESIGNS):
        blk = slice(k * SRV_BLOCK, (k + 1) * SRV_BLOCK)
        if cols is None:
            W[blk, :] = 3
        else:
            W[blk, list(cols)] = 3
            b[list(cols)] = 1
    return W, b


def srv_int_rows(rows, seed=0):
    """-> (f32 [rows, K] with entries in {0, 1, 2}, row r inside block r % 12, design index per row)"""
    rs = np.random.RandomState(6100 + rows + seed)
    X = np.zeros((rows, SRV_K), np.float32)
    which = np.arange(rows) % len(SRV_DESIGNS)
    for r in range(rows):
        pos = rs.choice(SRV_BLOCK, 1 + rs.randint(8), replace=False)
        X[r, which[r] * SRV_BLOCK + pos] = rs.randint(1, 3, len(pos))
    return X, which


def srv_random_rows(rows):
    """f16-valued random rows for the margin-guarded comparison (seed and scale chosen on the CPU: tests/test_tail_ref.py shows that
    fewer than 1 % of the rows fall under the margin)"""
    return np.random.RandomState(6200).randn(rows, SRV_K).astype(np.float16).astype(np.float32)


# ------------------------------------------------------------------------------------------------- mobile fused head, exact
MOB_K, MOB_C, MOB_BLOCK = 120, 6625, 10
MOB_DESIGNS = (
    ("first", (0,)), ("last", (6624,)), ("group_end", (127,)), ("group_start", (128,)), ("tie_127_128", (127, 128)),
    ("tie_two_groups", (5, 133, 261, 517)), ("tie_tiles_31_32", (31, 32)), ("tie_half_waves", (3, 4)), ("tie_lanes", (1, 65)),
    ("tie_first_last", (5, 6624)), ("last_group", (6527, 6528)), ("all_equal", None),
)
# rows of the issue -> (lines, line width): the mobile recognizer makes ((w - 1) // 2 // 2 + 1) // 2 steps of a w-wide line
MOB_SHAPES = {1: (1, 8), 3: (1, 24), 4: (1, 32), 5: (1, 40), 255: (51, 40), 256: (64, 32), 257: (257, 8)}
MOB_H = 48


def _int_head(K, C, block, designs, seed):
    rs = np.random.RandomState(seed)
    W = rs.randint(-2, 3, (K, C)).astype(np.float32)
    b = (rs.rand(C) < 0.5).astype(np.float32)
    b[0] = 1
    for k, (_, cols) in enumerate(designs):
        blk = slice(k * block, (k + 1) * block)
        if cols is None:
            W[blk, :] = 3
        else:
            W[blk, list(cols)] = 3
            b[list(cols)] = 1
    return W, b


def mob_int_head():
    """srv_int_head's construction at the mobile head's K = 120: twelve blocks of ten input channels"""
    return _int_head(MOB_K, MOB_C, MOB_BLOCK, MOB_DESIGNS, 6300)


def mob_int_rows(rows, seed=0):
    """-> (f32 [rows, K] of zeros and ones, row r inside block r % 12, design index per row)"""
    rs = np.random.RandomState(6400 + rows + seed)
    X = np.zeros((rows, MOB_K), np.float32)
    which = (np.arange(rows) + seed) % len(MOB_DESIGNS)
    for r in range(rows):
        pos = rs.choice(MOB_BLOCK, 1 + rs.randint(8), replace=False)
        X[r, which[r] * MOB_BLOCK + pos] = 1
    return X, which


def mob_random_rows(rows):
    """f16-valued random rows for the margin-guarded comparison of the mobile fused head"""
    return np.random.RandomState(6500).randn(rows, MOB_K).astype(np.float16).astype(np.float32)


# mutation -> (family, case) on which the reference changes (tests/test_tail_ref.py) and the device must disagree with it
KILLED_BY = {
    "last_maximum": ("head", "ties_C129"),
    "tie_to_later_group": ("head", "ties_C257"),
    "drop_partial_group": ("head", "ties_C129"),
    "collapse_across_blank": ("collapse", "n65_T40"),
    "score_over_stored": ("collapse", "n65_T40"),
    "open_last_run": ("collapse", "n65_T40"),
}
