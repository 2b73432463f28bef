"""ctypes binding of include/ocr_hip.h (plumbing for tests and bench.py).

Fails loudly when the HIP library is missing or no gfx950 device is visible: there is no
CPU fallback anywhere in the product path.
"""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LIB_PATH = os.environ.get("OCR_LIB_PATH") or os.path.join(HERE, "lib", "libocr_hip.so")   # (override: A/B runs against another build)
MODELS = os.path.join(ROOT, "models")

_lib = None


class OcrError(RuntimeError):
    pass


class ocr_img(C.Structure):
    _fields_ = [("data", C.c_void_p), ("rows", C.c_int), ("cols", C.c_int), ("row_stride", C.c_size_t)]


class ocr_det_cfg(C.Structure):
    _fields_ = [("model_dir", C.c_char_p), ("device_id", C.c_int), ("limit_type", C.c_char_p),
                ("limit_side_len", C.c_int), ("det_db_thresh", C.c_double), ("det_db_box_thresh", C.c_double),
                ("det_db_unclip_ratio", C.c_double), ("det_db_score_mode", C.c_char_p), ("use_dilation", C.c_int),
                ("precision", C.c_char_p), ("max_batch", C.c_int), ("cv_compat", C.c_int)]


CV_45, CV_410 = 45, 410  # ocr_det_cfg.cv_compat (0 = default = OCR_CV_COMPAT from the environment, else CV_410)


POST_REC_FLOATS, POST_REC_FILL = 12, 0xFFFFFFFF  # OCR_POST_REC_FLOATS / OCR_POST_REC_FILL


class ocr_post_stages(C.Structure):
    _fields_ = [("cap_pixels", C.c_size_t), ("cap_borders", C.c_int), ("cap_verts", C.c_int), ("bitmap", C.c_void_p),
                ("starts", C.c_void_p), ("npts", C.c_void_p), ("voff", C.c_void_p), ("verts", C.c_void_p),
                ("cand_valid", C.c_void_p), ("cand_boxes", C.c_void_p), ("record", C.c_void_p),
                ("rows", C.c_int), ("cols", C.c_int), ("ncont_all", C.c_int), ("ncont", C.c_int), ("nverts", C.c_int)]


class ocr_cls_cfg(C.Structure):
    _fields_ = [("model_dir", C.c_char_p), ("device_id", C.c_int), ("cls_thresh", C.c_double),
                ("cls_batch_num", C.c_int), ("precision", C.c_char_p)]


class ocr_rec_cfg(C.Structure):
    _fields_ = [("model_dir", C.c_char_p), ("device_id", C.c_int), ("label_path", C.c_char_p),
                ("rec_batch_num", C.c_int), ("rec_img_h", C.c_int), ("rec_img_w", C.c_int),
                ("precision", C.c_char_p), ("sort_mode", C.c_int)]


# every symbol include/ocr_hip.h declares (tests check the .so exports all of them)
EXPORTS = [
    "ocr_last_error", "ocr_rt_init", "ocr_rt_device_count", "ocr_rt_set_wait_mode", "ocr_rt_get_wait_mode",
    "ocr_det_cfg_default", "ocr_det_create", "ocr_det_destroy", "ocr_det_run", "ocr_det_run_batch",
    "ocr_det_last_shape", "ocr_det_prob_map", "ocr_det_bitmap", "ocr_det_resized", "ocr_det_post",
    "ocr_det_post_stages",
    "ocr_cls_cfg_default", "ocr_cls_create", "ocr_cls_destroy", "ocr_cls_run", "ocr_cls_probs",
    "ocr_rec_cfg_default", "ocr_rec_create", "ocr_rec_destroy", "ocr_rec_run", "ocr_rec_label",
    "ocr_rec_num_classes", "ocr_rec_steps", "ocr_rec_run_chars", "ocr_rec_logits_row", "ocr_selftest_topk",
    "ocr_rec_set_launch_lines", "ocr_rec_timing", "ocr_rec_timing_report",
    "ocr_net_create", "ocr_net_create_precision", "ocr_net_destroy", "ocr_net_forward", "ocr_net_forward_ragged", "ocr_net_forward_ragged_images", "ocr_net_num_tensors", "ocr_net_tensor_exists", "ocr_net_fetch",
    "ocr_net_timing", "ocr_net_timing_report", "ocr_probe", "ocr_selftest_refuse_launch", "ocr_selftest_lds_memo",
    "ocr_selftest_unclip", "ocr_selftest_unclip_box",
    "ocr_selftest_det_pre", "ocr_selftest_line_pre", "ocr_selftest_line_pre_ragged",
    "ocr_selftest_warp_crops", "ocr_selftest_rotate180_groups", "ocr_selftest_crop_plan", "ocr_selftest_rotation_groups",
    "ocr_selftest_softmax_argmax", "ocr_selftest_head_combine", "ocr_selftest_srv_argmax", "ocr_selftest_ctc_reduce",
    "ocr_selftest_ctc", "ocr_selftest_topk_lines", "ocr_selftest_rec_head",
    "ocr_srv_net_create", "ocr_srv_net_destroy", "ocr_srv_net_forward", "ocr_srv_net_rerun", "ocr_srv_net_num_tensors", "ocr_srv_net_fetch",
    "ocr_srv_net_timing", "ocr_srv_net_timing_report", "ocr_srv_net_num_launches", "ocr_srv_net_launch_info", "ocr_srv_net_run_launches",
    "ocr_srv_net_upload", "ocr_srv_net_set_ctc", "ocr_srv_net_ctc_tail",
    "ocr_srv_net_create_plan", "ocr_srv_net_set_config", "ocr_srv_gemm_num_configs", "ocr_srv_gemm_config_name", "ocr_srv_gemm_config_bn",
]


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise OcrError("libocr_hip.so is not built (%s): run __graft_entry__.build()" % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        L.ocr_last_error.restype = C.c_char_p
        L.ocr_net_create.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.POINTER(C.c_void_p)]
        L.ocr_net_create_precision.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.c_char_p, C.POINTER(C.c_void_p)]
        L.ocr_net_destroy.argtypes = [C.c_void_p]
        L.ocr_net_forward.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]
        if hasattr(L, "ocr_net_forward_ragged_images"):
            L.ocr_net_forward_ragged_images.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
        if hasattr(L, "ocr_net_forward_ragged"):
            L.ocr_net_forward_ragged.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int]
        L.ocr_net_num_tensors.argtypes = [C.c_void_p]
        L.ocr_net_tensor_exists.argtypes = [C.c_void_p, C.c_int]
        L.ocr_net_fetch.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_int)]
        L.ocr_net_timing.argtypes = [C.c_void_p, C.c_int]
        L.ocr_net_timing_report.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t]
        L.ocr_probe.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        if hasattr(L, "ocr_selftest_refuse_launch"):
            L.ocr_selftest_refuse_launch.argtypes = [C.c_char_p]
        _lib = L
    return _lib


def check(rc):
    if rc != 0:
        raise OcrError("libocr_hip error %d: %s" % (rc, lib().ocr_last_error().decode(errors="replace")))


def _raise(L, rc, out):
    err = OcrError("libocr_hip error %d: %s" % (rc, L.ocr_last_error().decode(errors="replace")))
    err.code = rc
    err.out = out  # the buffer as the call left it
    raise err


def _decode_frame(name, c, h, w, device_id, fill=0, cap=None):
    """L.<name>(&c, device_id, bgr, cap) - the ocr_X_decode of a format route - into an (h, w, 3) buffer pre-filled with `fill`;
    (1, 1, 3) where h x w is no image size: the library refuses the descriptor before it looks at the capacity.  cap: the
    capacity the call is told, when it is not the buffer's size"""
    L = lib()
    fn = getattr(L, name)
    fn.argtypes = [C.POINTER(type(c)), C.c_int, C.c_void_p, C.c_size_t]
    out = np.full((h, w, 3) if 0 < h and 0 < w and h * w <= (64 << 20) else (1, 1, 3), fill, np.uint8)
    rc = fn(C.byref(c), device_id, out.ctypes.data, out.size if cap is None else cap)
    if rc != 0:
        _raise(L, rc, out)
    return out


def _time_coded(name, coded, iters, device_id, single):
    """L.<name>_batch over the descriptors of `coded` as one batch (single: L.<name> of the first): three phases in ms"""
    L = lib()
    ctype = type(coded[0].c)
    ms = (C.c_double * 3)()
    if single:
        fn = getattr(L, name)
        fn.argtypes = [C.POINTER(ctype), C.c_int, C.c_int, C.POINTER(C.c_double)]
        rc = fn(C.byref(coded[0].c), device_id, iters, ms)
    else:
        fn = getattr(L, name + "_batch")
        fn.argtypes = [C.POINTER(C.POINTER(ctype)), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double)]
        ptrs = (C.POINTER(ctype) * len(coded))(*[C.pointer(k.c) for k in coded])
        rc = fn(ptrs, len(coded), device_id, iters, ms)
    if rc != 0:
        _raise(L, rc, None)
    return list(ms)


class SrvNet:
    """raw taps of a server network (BASELINE configs[4]; hand-written plans, seeded weights): kind "det" | "rec" """

    def __init__(self, kind, precision="fp16", model_dir=None, device=0):
        L = self._lib()
        if model_dir is None:
            root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
            model_dir = os.path.join(root, "models_server", kind)
        self.h = C.c_void_p()
        check(L.ocr_srv_net_create(kind.encode(), model_dir.encode(), device, precision.encode(), C.byref(self.h)))
        self.shape = None

    @staticmethod
    def _lib():
        L = lib()
        L.ocr_srv_net_create.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_char_p, C.POINTER(C.c_void_p)]
        L.ocr_srv_net_create_plan.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_char_p, C.POINTER(C.c_void_p)]
        L.ocr_srv_net_set_config.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.ocr_srv_net_destroy.argtypes = [C.c_void_p]
        L.ocr_srv_net_forward.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]
        L.ocr_srv_net_rerun.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]
        L.ocr_srv_net_num_tensors.argtypes = [C.c_void_p]
        L.ocr_srv_net_fetch.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_int)]
        L.ocr_srv_net_timing.argtypes = [C.c_void_p, C.c_int]
        L.ocr_srv_net_timing_report.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t]
        L.ocr_srv_net_num_launches.argtypes = [C.c_void_p]
        L.ocr_srv_net_launch_info.argtypes = [C.c_void_p, C.c_int, C.c_char_p, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int)]
        L.ocr_srv_net_run_launches.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.ocr_srv_net_upload.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]
        return L

    @classmethod
    def from_plan(cls, plan, params_path, precision="fp16", device=0):
        """test hook: a network on the caller's plan text and parameter file (tools/synth_weights.py's .pdiparams format, records =
        the plan's `# param` names in sorted order).  OcrError.code tells a bad plan (-1) from a missing parameter (-2)"""
        L = cls._lib()
        self = cls.__new__(cls)
        self.h = C.c_void_p()
        self.shape = None
        rc = L.ocr_srv_net_create_plan(None if plan is None else plan.encode(), None if params_path is None else os.fsencode(params_path),
                                       device, precision.encode(), C.byref(self.h))
        if rc != 0:
            self.h = None
            _raise(L, rc, None)
        return self

    @staticmethod
    def configs():
        """the GEMM family's tile configurations, from the library: [(id, name, column-tile width)]"""
        L = lib()
        L.ocr_srv_gemm_config_name.restype = C.c_char_p
        L.ocr_srv_gemm_config_name.argtypes = [C.c_int]
        L.ocr_srv_gemm_config_bn.argtypes = [C.c_int]
        return [(i, L.ocr_srv_gemm_config_name(i).decode(), L.ocr_srv_gemm_config_bn(i)) for i in range(L.ocr_srv_gemm_num_configs())
                if L.ocr_srv_gemm_config_name(i)]

    def set_config(self, cfg, strict=True):
        """test hook: every GEMM launch of this net on tile configuration `cfg` (-1: the default choice); the next forward re-binds.
        strict: a launch the configuration cannot run makes that forward raise (OcrError.code -1) instead of falling back"""
        L = lib()
        rc = L.ocr_srv_net_set_config(self.h, cfg, 1 if strict else 0)
        if rc != 0:
            _raise(L, rc, None)

    def forward(self, x, keep_all=False):
        x = np.ascontiguousarray(x, dtype=np.float32)
        n, h, w, c = x.shape
        assert c == 3
        self.shape = (n, h, w)
        rc = lib().ocr_srv_net_forward(self.h, x.ctypes.data, n, h, w, 1 if keep_all else 0)
        if rc != 0:
            _raise(lib(), rc, None)
        return self.fetch(-1)

    def rerun(self, iters=1):
        n, h, w = self.shape
        check(lib().ocr_srv_net_rerun(self.h, n, h, w, iters))

    def num_tensors(self):
        return lib().ocr_srv_net_num_tensors(self.h)

    def fetch(self, tid, cap=None):
        dims = (C.c_int * 4)()
        cap = cap or (1 << 22)
        while True:
            out = np.empty(cap, np.float32)
            rc = lib().ocr_srv_net_fetch(self.h, tid, out.ctypes.data, cap, dims)
            if rc == -4:
                cap *= 8
                continue
            check(rc)
            break
        n = dims[0] * dims[1] * dims[2] * dims[3]
        return out[:n].reshape(dims[0], dims[1], dims[2], dims[3]).copy()

    def launches(self):
        """test hook: the launch list of the last forward's binding as (name, output tid, [input tids])"""
        out = []
        name = C.create_string_buffer(256)
        o, n_in, ins = C.c_int(), C.c_int(), (C.c_int * 8)()
        for i in range(lib().ocr_srv_net_num_launches(self.h)):
            check(lib().ocr_srv_net_launch_info(self.h, i, name, len(name), C.byref(o), ins, 8, C.byref(n_in)))
            out.append((name.value.decode(), o.value, [ins[k] for k in range(n_in.value)]))
        return out

    def run_launches(self, first, count=1):
        """test hook: launches [first, first + count) of the last forward's binding, alone"""
        check(lib().ocr_srv_net_run_launches(self.h, first, count))

    def upload(self, tid, x):
        """test hook: logical NHWC data into tensor `tid` (rounded to its element type, pad channels zero)"""
        x = np.ascontiguousarray(x, dtype=np.float32)
        check(lib().ocr_srv_net_upload(self.h, tid, x.ctypes.data, x.size))

    def set_ctc(self, on=True):
        """test hook: the CTC head's partial mode (f16 build), as the recognizer stage switches it; the next forward re-binds"""
        L = lib()
        L.ocr_srv_net_set_ctc.argtypes = [C.c_void_p, C.c_int]
        check(L.ocr_srv_net_set_ctc(self.h, 1 if on else 0))

    def ctc_tail(self):
        """test hook: the stage's tail launch on the output of the current binding -> (amax int32 [rows], pmax f32 [rows], slots, step)"""
        L = lib()
        L.ocr_srv_net_ctc_tail.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_long, C.POINTER(C.c_long), C.POINTER(C.c_int),
                                           C.POINTER(C.c_int)]
        cap = 1 << 16
        a, p = np.zeros(cap, np.int32), np.zeros(cap, np.float32)
        rows, slots, step = C.c_long(), C.c_int(), C.c_int()
        check(L.ocr_srv_net_ctc_tail(self.h, a.ctypes.data, p.ctypes.data, cap, C.byref(rows), C.byref(slots), C.byref(step)))
        return a[:rows.value].copy(), p[:rows.value].copy(), slots.value, step.value

    def timing(self, on=True):
        check(lib().ocr_srv_net_timing(self.h, 1 if on else 0))

    def timing_report(self):
        buf = C.create_string_buffer(1 << 18)
        check(lib().ocr_srv_net_timing_report(self.h, buf, len(buf)))
        rep = {}
        for line in buf.value.decode().splitlines():
            name, ms, cnt, fl, by = line.rsplit(" ", 4)
            rep[name] = dict(ms=float(ms), count=int(cnt), flops=float(fl), bytes=float(by))
        return rep

    def close(self):
        if self.h:
            lib().ocr_srv_net_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def selftest_unclip(quads, deltas, cap=64):
    """device ClipperOffset (jtRound, closed polygon) of n int quads -> list of [k][2] int64 arrays (None: scratch overflow)"""
    quads = np.ascontiguousarray(quads, dtype=np.int32).reshape(-1, 8)
    deltas = np.ascontiguousarray(deltas, dtype=np.float64)
    n = quads.shape[0]
    out = np.zeros((n, cap, 2), np.int64)
    counts = np.zeros(n, np.int32)
    trig = np.zeros((n, 3), np.float64)
    L = lib()
    L.ocr_selftest_unclip.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    check(L.ocr_selftest_unclip(quads.ctypes.data, deltas.ctypes.data, n, out.ctypes.data, cap, counts.ctypes.data, trig.ctypes.data))
    return out, counts, trig


def selftest_unclip_box(boxes, unclip_ratio):
    """device UnClip -> minAreaRect -> GetMiniBoxes of n float boxes -> (out14 [n,14], status [n,2])"""
    boxes = np.ascontiguousarray(boxes, dtype=np.float32).reshape(-1, 8)
    n = boxes.shape[0]
    out = np.zeros((n, 14), np.float32)
    st = np.zeros((n, 2), np.int32)
    L = lib()
    L.ocr_selftest_unclip_box.argtypes = [C.c_void_p, C.c_float, C.c_int, C.c_void_p, C.c_void_p]
    check(L.ocr_selftest_unclip_box(boxes.ctypes.data, float(unclip_ratio), n, out.ctypes.data, st.ctypes.data))
    return out, st


def selftest_topk(rows, p0, k, ncols=None):
    """the top-k kernel alone (ocr_selftest_topk): rows [n, pitch] f32 of which the first ncols columns are a logits row, p0 [n]
    the rank-0 probability -> (ids [n, k] int32, probs [n, k] f32); ranks a row does not have: id -1, prob 0"""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    assert rows.ndim == 2
    n, pitch = rows.shape
    C_ = pitch if ncols is None else int(ncols)
    p0 = np.ascontiguousarray(p0, dtype=np.float32).reshape(n)
    ids = np.zeros((n, k), np.int32)
    probs = np.zeros((n, k), np.float32)
    L = lib()
    L.ocr_selftest_topk.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                    C.c_void_p, C.c_void_p]
    check(L.ocr_selftest_topk(rows.ctypes.data, n, C_, pitch, p0.ctypes.data, int(k), ids.ctypes.data, probs.ctypes.data))
    return ids, probs


SELFTEST_FILL, SELFTEST_GUARD = 0xA5, 256   # include/ocr_hip.h OCR_SELFTEST_FILL / OCR_SELFTEST_GUARD
PAD_REC, PAD_CLS = 0, 1                      # OCR_PAD_REC / OCR_PAD_CLS
STAGE_REC, STAGE_CLS = 1, 2                  # OCR_STAGE_REC / OCR_STAGE_CLS


def _split_guard(raw, count, dtype):
    """the first `count` elements of a self-test output and the guard bytes behind them"""
    n = count * np.dtype(dtype).itemsize
    return raw[:n].view(dtype), raw[n:]


def selftest_det_pre(buf, src_offset, src_stride, src_image_bytes, N, sh, sw, dh, dw):
    """launch_det_pre alone (ocr_selftest_det_pre): buf a flat uint8 buffer; image i at byte src_offset + i * src_image_bytes of its
    256-byte-aligned device copy -> (f32 [N, dh, dw, 3], u8 tap [N, dh, dw, 3], guard bytes behind the f32, guard bytes behind the tap)"""
    buf = np.ascontiguousarray(buf, dtype=np.uint8).reshape(-1)
    cnt = max(0, N) * max(0, dh) * max(0, dw) * 3
    if cnt > 1 << 26:
        cnt = 0  # (the call refuses such sizes before it writes)
    out = np.zeros(cnt * 4 + SELFTEST_GUARD, np.uint8)
    res = np.zeros(cnt + SELFTEST_GUARD, np.uint8)
    L = lib()
    L.ocr_selftest_det_pre.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int,
                                       C.c_int, C.c_void_p, C.c_void_p]
    check(L.ocr_selftest_det_pre(buf.ctypes.data, buf.size, int(src_offset), int(src_stride), int(src_image_bytes), int(N), int(sh),
                                 int(sw), int(dh), int(dw), out.ctypes.data, res.ctypes.data))
    x, gx = _split_guard(out, cnt, np.float32)
    r, gr = _split_guard(res, cnt, np.uint8)
    return x.reshape(N, dh, dw, 3), r.reshape(N, dh, dw, 3), gx, gr


def _parent_rows(img):
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 2 and img.flags.c_contiguous, "parent image: uint8 [rows, stride] with the pad bytes"
    return img


def selftest_line_pre(parent, cols, lines, imgH, imgW, nslots, pad_mode, stage=STAGE_REC):
    """launch_line_pre alone (ocr_selftest_line_pre): parent uint8 [rows, stride] holding `cols` BGR pixels per row; lines: rows of
    (x, y, w, h, resize_w, slot) -> (f32 [nslots, imgH, imgW, 3], guard bytes behind it)"""
    parent = _parent_rows(parent)
    lines = np.ascontiguousarray(lines, dtype=np.int32).reshape(-1, 6)
    cnt = max(0, nslots) * max(0, imgH) * max(0, imgW) * 3
    if cnt > 1 << 26:
        cnt = 0
    out = np.zeros(cnt * 4 + SELFTEST_GUARD, np.uint8)
    L = lib()
    L.ocr_selftest_line_pre.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_size_t, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                        C.c_int, C.c_void_p]
    check(L.ocr_selftest_line_pre(parent.ctypes.data, parent.shape[0], int(cols), parent.shape[1], lines.ctypes.data, len(lines), int(imgH),
                                  int(imgW), int(nslots), int(pad_mode), int(stage), out.ctypes.data))
    x, g = _split_guard(out, cnt, np.float32)
    return x.reshape(nslots, imgH, imgW, 3), g


def selftest_line_pre_ragged(parent, cols, lines, imgH, stage=STAGE_REC):
    """launch_line_pre_ragged alone (ocr_selftest_line_pre_ragged): lines: rows of (x, y, w, h, resize_w, tensor_w) -> (list of f32
    [imgH, tensor_w, 3] per line, guard bytes behind the last)"""
    parent = _parent_rows(parent)
    lines = np.ascontiguousarray(lines, dtype=np.int32).reshape(-1, 6)
    ok = imgH > 0 and len(lines) and (lines[:, 5] > 0).all() and (lines[:, 5] <= 8192).all() and imgH <= 8192
    widths = [int(w) for w in lines[:, 5]] if ok else []
    cnt = imgH * sum(widths) * 3 if ok else 0
    if cnt > 1 << 26:
        cnt, widths = 0, []
    out = np.zeros(cnt * 4 + SELFTEST_GUARD, np.uint8)
    L = lib()
    L.ocr_selftest_line_pre_ragged.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_size_t, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    check(L.ocr_selftest_line_pre_ragged(parent.ctypes.data, parent.shape[0], int(cols), parent.shape[1], lines.ctypes.data, len(lines),
                                         int(imgH), int(stage), out.ctypes.data))
    x, g = _split_guard(out, cnt, np.float32)
    outs, at = [], 0
    for w in widths:
        outs.append(x[at:at + imgH * w * 3].reshape(imgH, w, 3))
        at += imgH * w * 3
    return outs, g


# ---- the crop geometry between detector and recognizer alone (include/ocr_hip.h)
class ocr_warp_case(C.Structure):
    _fields_ = [("src_off", C.c_uint64), ("sstride", C.c_uint64), ("sw", C.c_int32), ("sh", C.c_int32), ("dw", C.c_int32), ("dh", C.c_int32),
                ("rot", C.c_int32), ("bw0", C.c_int32), ("m", C.c_double * 9)]


def selftest_warp_crops(src, crops, max_pixels, out_off, out_bytes):
    """ONE launch_warp_crops (ocr_selftest_warp_crops): src a flat uint8 buffer; crops: dicts with src_off, sstride, sw, sh, dw, dh, rot,
    bw0 and m (9 doubles, destination -> source); crop k writes dw * dh * 3 bytes at out_off[k] of an output of out_bytes bytes ->
    (uint8 [out_bytes] with the fill wherever nothing was written, guard bytes behind it)"""
    src = np.ascontiguousarray(src, dtype=np.uint8).reshape(-1)
    n = len(crops)
    arr = (ocr_warp_case * max(1, n))()
    for k, c in enumerate(crops):
        arr[k] = ocr_warp_case(int(c["src_off"]), int(c["sstride"]), int(c["sw"]), int(c["sh"]), int(c["dw"]), int(c["dh"]), int(c["rot"]),
                               int(c["bw0"]), (C.c_double * 9)(*[float(v) for v in c["m"]]))
    off = np.ascontiguousarray(out_off, dtype=np.uint64).reshape(-1)
    assert off.size == n
    if n == 0:
        off = np.zeros(1, np.uint64)
    cnt = int(out_bytes) if 0 < out_bytes <= 1 << 28 else 0
    out = np.zeros(cnt + SELFTEST_GUARD, np.uint8)
    _tail_call("ocr_selftest_warp_crops", [C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p],
               src.ctypes.data, src.size, C.addressof(arr), n, int(max_pixels), off.ctypes.data, int(out_bytes), out.ctypes.data)
    return out[:cnt], out[cnt:]


def selftest_rotate180_groups(buf, rois, seg):
    """ONE launch_rotate180_groups (ocr_selftest_rotate180_groups) on a copy of the flat uint8 buffer `buf`; rois: rows of (byte offset of
    the view, stride, x, y, w, h) in launch order; seg: the ngroups + 1 offsets into rois -> the whole buffer afterwards"""
    buf = np.ascontiguousarray(buf, dtype=np.uint8).reshape(-1).copy()
    rois = np.ascontiguousarray(rois, dtype=np.int64).reshape(-1, 6)
    seg = np.ascontiguousarray(seg, dtype=np.int32).reshape(-1)
    assert seg.size >= 1
    _tail_call("ocr_selftest_rotate180_groups", [C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p, C.c_int],
               buf.ctypes.data, buf.size, rois.ctypes.data, len(rois), seg.ctypes.data, seg.size - 1)
    return buf


CROP_PLAN_FIELDS = ("left", "top", "sw", "sh", "dw", "dh", "rot", "orows", "ocols", "bw0")


def selftest_crop_plan(rows, cols, box):
    """plan_rotate_crop of csrc/crop.h for one box (ocr_selftest_crop_plan, host only) -> dict of CROP_PLAN_FIELDS and minv (float64 [9])"""
    b = np.ascontiguousarray(np.asarray(box, np.int32).reshape(8))
    f = np.zeros(len(CROP_PLAN_FIELDS), np.int32)
    minv = np.zeros(9, np.float64)
    _tail_call("ocr_selftest_crop_plan", [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p], int(rows), int(cols), b.ctypes.data,
               f.ctypes.data, minv.ctypes.data)
    p = {k: int(v) for k, v in zip(CROP_PLAN_FIELDS, f)}
    p["minv"] = minv
    return p


def selftest_rotation_groups(rects, views):
    """the grouping the 180-degree rotations are launched with (ocr_selftest_rotation_groups, host only): rects rows of (x, y, w, h),
    views[i] the view rectangle i lies in -> (order: request indices group after group, seg: ngroups + 1 offsets into order)"""
    r = np.ascontiguousarray(rects, dtype=np.int32).reshape(-1, 4)
    v = np.ascontiguousarray(views, dtype=np.int32).reshape(-1)
    assert v.size == len(r)
    order = np.zeros(max(1, len(r)), np.int32)
    seg = np.zeros(len(r) + 1, np.int32)
    ng = C.c_int(0)
    _tail_call("ocr_selftest_rotation_groups", [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_int)],
               r.ctypes.data, v.ctypes.data, len(r), order.ctypes.data, seg.ctypes.data, C.byref(ng))
    return [int(k) for k in order[:len(r)]], [int(s) for s in seg[:ng.value + 1]]


# ---- the recognizer's tail launches alone (include/ocr_hip.h): every output comes back as (values, guard bytes)
def _tail_buf(count):
    return np.zeros(max(0, int(count)) * 4 + SELFTEST_GUARD, np.uint8)


def _tail_ptr(a):
    return None if a is None else a.ctypes.data


def _tail_call(name, argtypes, *args):
    L = lib()
    fn = getattr(L, name)
    fn.argtypes = argtypes
    rc = fn(*args)
    if rc != 0:
        _raise(L, rc, None)


def selftest_softmax_argmax(logits, probs=False):
    """launch_softmax_argmax on f32 [rows, C] -> {"amax": (int32 [rows], guard), "pmax": (f32 [rows], guard), "probs": (f32 [rows, C],
    guard) when asked for}"""
    x = np.ascontiguousarray(logits, dtype=np.float32)
    rows, C_ = x.shape
    ok = 0 < rows * C_ <= 1 << 26
    q = _tail_buf(rows * C_ if ok else 0) if probs else None
    a, p = _tail_buf(rows), _tail_buf(rows)
    _tail_call("ocr_selftest_softmax_argmax", [C.c_void_p, C.c_long, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p],
               x.ctypes.data, rows, C_, _tail_ptr(q), a.ctypes.data, p.ctypes.data)
    out = {"amax": _split_guard(a, rows, np.int32), "pmax": _split_guard(p, rows, np.float32)}
    if probs:
        v, g = _split_guard(q, rows * C_, np.float32)
        out["probs"] = (v.reshape(rows, C_), g)
    return out


def selftest_head_combine(hmax, hsum, hidx):
    """launch_head_combine on [rows, groups] partials -> ((amax, guard), (pmax, guard))"""
    m = np.ascontiguousarray(hmax, dtype=np.float32)
    s = np.ascontiguousarray(hsum, dtype=np.float32)
    i = np.ascontiguousarray(hidx, dtype=np.int32)
    assert m.ndim == 2 and m.shape == s.shape == i.shape
    rows, G = m.shape
    a, p = _tail_buf(rows), _tail_buf(rows)
    _tail_call("ocr_selftest_head_combine", [C.c_void_p, C.c_void_p, C.c_void_p, C.c_long, C.c_int, C.c_void_p, C.c_void_p],
               m.ctypes.data, s.ctypes.data, i.ctypes.data, rows, G, a.ctypes.data, p.ctypes.data)
    return _split_guard(a, rows, np.int32), _split_guard(p, rows, np.float32)


def selftest_srv_argmax(logits, ncols=None, one_pass=False):
    """srv::launch_argmax_softmax on f32 [rows, ld] of which the first ncols columns are the logits -> ((amax, guard), (pmax, guard))"""
    x = np.ascontiguousarray(logits, dtype=np.float32)
    rows, ld = x.shape
    a, p = _tail_buf(rows), _tail_buf(rows)
    _tail_call("ocr_selftest_srv_argmax", [C.c_void_p, C.c_long, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p],
               x.ctypes.data, rows, ld if ncols is None else int(ncols), ld, 1 if one_pass else 0, a.ctypes.data, p.ctypes.data)
    return _split_guard(a, rows, np.int32), _split_guard(p, rows, np.float32)


def selftest_ctc_reduce(part, step=1):
    """srv::launch_ctc_reduce on f32 [rows, slots, 4] partials (the index as int bits) -> ((amax, guard), (pmax, guard))"""
    x = np.ascontiguousarray(part, dtype=np.float32)
    rows, slots, four = x.shape
    assert four == 4
    a, p = _tail_buf(rows), _tail_buf(rows)
    _tail_call("ocr_selftest_ctc_reduce", [C.c_void_p, C.c_long, C.c_int, C.c_int, C.c_void_p, C.c_void_p],
               x.ctypes.data, rows, slots, int(step), a.ctypes.data, p.ctypes.data)
    return _split_guard(a, rows, np.int32), _split_guard(p, rows, np.float32)


def selftest_ctc(amax, pmax, max_len, T=None, lines=None, chars=False):
    """launch_ctc (T given) / launch_ctc_ragged (lines: rows of (first step, steps)) / launch_ctc_chars (chars) on flat step arrays
    -> dict of (values, guard): ids [n, max_len], lens [n], scores [n] and, with chars, steps / nsteps / probs [n, max_len]"""
    am = np.ascontiguousarray(amax, dtype=np.int32).reshape(-1)
    pm = np.ascontiguousarray(pmax, dtype=np.float32).reshape(-1)
    assert am.size == pm.size
    if lines is not None:
        lines = np.ascontiguousarray(lines, dtype=np.int32).reshape(-1, 2)
        n = len(lines)
    else:
        n = am.size // T if T and T > 0 else 0
    nch = n * max_len if 0 < n and 0 < max_len <= 4096 and n <= 1 << 18 else 0
    nl = n if nch else 0
    bufs = {"ids": _tail_buf(nch), "lens": _tail_buf(nl), "scores": _tail_buf(nl)}
    if chars:
        bufs.update(steps=_tail_buf(nch), nsteps=_tail_buf(nch), probs=_tail_buf(nch))
    _tail_call("ocr_selftest_ctc", [C.c_void_p, C.c_void_p, C.c_long, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 6,
               am.ctypes.data, pm.ctypes.data, am.size, n, int(T or 0), _tail_ptr(lines), int(max_len), 1 if chars else 0,
               bufs["ids"].ctypes.data, bufs["lens"].ctypes.data, bufs["scores"].ctypes.data, _tail_ptr(bufs.get("steps")),
               _tail_ptr(bufs.get("nsteps")), _tail_ptr(bufs.get("probs")))
    out = {}
    for k, b in bufs.items():
        per_char = k in ("ids", "steps", "nsteps", "probs")
        v, g = _split_guard(b, nch if per_char else nl, np.float32 if k in ("scores", "probs") else np.int32)
        out[k] = (v.reshape(n, max_len) if per_char else v, g)
    return out


def selftest_topk_lines(rows, T, lens, steps, p0, k, ncols=None):
    """launch_ctc_topk on nlines lines of T rows: rows f32 [nlines * T, pitch]; lens [nlines]; steps, p0 [nlines, max_len] ->
    ((ids [nlines, max_len, k], guard), (probs likewise, guard))"""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    nrows, pitch = rows.shape
    lens = np.ascontiguousarray(lens, dtype=np.int32).reshape(-1)
    n = lens.size
    steps = np.ascontiguousarray(steps, dtype=np.int32).reshape(n, -1)
    max_len = steps.shape[1]
    p0 = np.ascontiguousarray(p0, dtype=np.float32).reshape(n, max_len)
    assert nrows == n * T
    cnt = n * max_len * k if 1 <= k <= 8 else 0
    ids, probs = _tail_buf(cnt), _tail_buf(cnt)
    _tail_call("ocr_selftest_topk_lines", [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                           C.c_int, C.c_void_p, C.c_void_p],
               rows.ctypes.data, n, int(T), pitch if ncols is None else int(ncols), pitch, lens.ctypes.data, steps.ctypes.data,
               p0.ctypes.data, max_len, int(k), ids.ctypes.data, probs.ctypes.data)
    (i, gi), (p, gp) = _split_guard(ids, cnt, np.int32), _split_guard(probs, cnt, np.float32)
    return (i.reshape(n, max_len, k), gi), (p.reshape(n, max_len, k), gp)


def selftest_rec_head(weights, precision, rows, lines, imgH, imgW, mode=0, ncols=6625, model_dir=None):
    """ocr_selftest_rec_head: the mobile recognizer's head through its binder on rows f32 [nrows, K] -> dict(amax=(int32 [nrows],
    guard), pmax=(f32 [nrows], guard), logits=f32 [nrows, C] or None, names=[the two launches' names])"""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    n, K = rows.shape
    if model_dir is None:
        model_dir = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "models", "rec")
    a, p = _tail_buf(n), _tail_buf(n)
    lg = np.zeros((n, ncols), np.float32) if mode else None
    nc = C.c_int()
    names = C.create_string_buffer(512)
    _tail_call("ocr_selftest_rec_head", [C.c_char_p, C.c_char_p, C.c_char_p, C.c_void_p, C.c_long, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.c_char_p, C.c_size_t],
               model_dir.encode(), None if weights is None else weights.encode(), precision.encode(), rows.ctypes.data, n, K, int(lines),
               int(imgH), int(imgW), int(mode), a.ctypes.data, p.ctypes.data, _tail_ptr(lg), C.byref(nc), names, len(names))
    assert nc.value == ncols
    return dict(amax=_split_guard(a, n, np.int32), pmax=_split_guard(p, n, np.float32), logits=lg, names=names.value.decode().split())


def probe(a, b):
    a = np.ascontiguousarray(a, dtype=np.float32)
    b = np.ascontiguousarray(b, dtype=np.float32)
    out = np.empty((8, a.size), dtype=np.float32)
    check(lib().ocr_probe(a.ctypes.data, b.ctypes.data, out.ctypes.data, a.size))
    return out


class Net:
    """Raw network tap (ocr_net_*): host f32 NHWC in, logical NHWC tensors out."""

    def __init__(self, kind, model_dir=None, weights=None, device=0, precision="fp32"):
        self.kind = kind
        model_dir = model_dir or os.path.join(MODELS, kind)
        self.h = C.c_void_p()
        check(lib().ocr_net_create_precision(kind.encode(), model_dir.encode(), weights.encode() if weights else None, device,
                                             precision.encode(), C.byref(self.h)))

    def forward(self, x_nhwc, keep_all=False):
        x = np.ascontiguousarray(x_nhwc, dtype=np.float32)
        n, h, w, c = x.shape
        assert c == 3
        check(lib().ocr_net_forward(self.h, x.ctypes.data, n, h, w, int(keep_all)))
        return self.fetch(-1)

    def forward_ragged(self, lines, keep_all=False):
        """lines: list of f32 [H, W_i, 3] arrays of one height -> the output's lines one after the other [1, 1, sum T_i, C]"""
        h = lines[0].shape[0]
        assert all(l.shape[0] == h and l.shape[2] == 3 for l in lines)
        x = np.concatenate([np.ascontiguousarray(l, dtype=np.float32).reshape(-1) for l in lines])
        widths = np.array([l.shape[1] for l in lines], dtype=np.int32)
        check(lib().ocr_net_forward_ragged(self.h, x.ctypes.data, len(lines), h, widths.ctypes.data, int(keep_all)))
        return self.fetch(-1)

    def forward_ragged_images(self, imgs, keep_all=False):
        """imgs: list of f32 [H_i, W_i, 3] arrays (sizes multiples of 32) -> the output's images one after the other"""
        x = np.concatenate([np.ascontiguousarray(l, dtype=np.float32).reshape(-1) for l in imgs])
        hs = np.array([l.shape[0] for l in imgs], dtype=np.int32)
        ws = np.array([l.shape[1] for l in imgs], dtype=np.int32)
        check(lib().ocr_net_forward_ragged_images(self.h, x.ctypes.data, len(imgs), hs.ctypes.data, ws.ctypes.data, int(keep_all)))
        return self.fetch(-1)

    def fetch(self, tid, cap=None):
        dims = (C.c_int * 4)()
        cap = cap or (1 << 28)
        # first call with a tiny buffer is not possible (no size query) -> allocate by trying sizes
        buf = np.empty(min(cap, 1 << 22), dtype=np.float32)
        rc = lib().ocr_net_fetch(self.h, tid, buf.ctypes.data, buf.size, dims)
        if rc == -4:
            n = dims[0] * dims[1] * dims[2] * dims[3]
            buf = np.empty(n, dtype=np.float32)
            rc = lib().ocr_net_fetch(self.h, tid, buf.ctypes.data, buf.size, dims)
        check(rc)
        n = dims[0] * dims[1] * dims[2] * dims[3]
        return buf[:n].reshape(dims[0], dims[1], dims[2], dims[3]).copy()

    def num_tensors(self):
        return lib().ocr_net_num_tensors(self.h)

    def exists(self, tid):
        """did the last forward write plan tensor `tid`? (a fused-away tensor never reaches device memory)"""
        return bool(lib().ocr_net_tensor_exists(self.h, int(tid)))

    def timing(self, on=True):
        check(lib().ocr_net_timing(self.h, int(on)))

    def timing_report(self):
        buf = C.create_string_buffer(1 << 16)
        check(lib().ocr_net_timing_report(self.h, buf, len(buf)))
        out = {}
        for line in buf.value.decode().splitlines():
            name, ms, cnt, fl, by = line.split()
            out[name] = dict(ms=float(ms), count=int(cnt), flops=float(fl), bytes=float(by))
        return out

    def close(self):
        if self.h:
            lib().ocr_net_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---------------------------------------------------------------------------------------------
# stage handles
# ---------------------------------------------------------------------------------------------
def _img(a):
    a = np.asarray(a)
    if a.size == 0:
        return ocr_img(None, 0, 0, 0)  # the library reports "Empty image data provided"
    assert a.dtype == np.uint8 and a.ndim == 3 and a.shape[2] == 3 and a.strides[2] == 1 and a.strides[1] == 3
    return ocr_img(a.ctypes.data, a.shape[0], a.shape[1], a.strides[0])


def _imgs(arrs):
    arr = (ocr_img * len(arrs))()
    for i, a in enumerate(arrs):
        arr[i] = _img(a)
    return arr


def _stage_protos(L):
    if getattr(L, "_stage_protos_done", False):
        return
    vp, ip = C.c_void_p, C.POINTER(C.c_int)
    L.ocr_det_cfg_default.argtypes = [C.POINTER(ocr_det_cfg)]
    L.ocr_det_create.argtypes = [C.POINTER(ocr_det_cfg), C.POINTER(vp)]
    L.ocr_det_destroy.argtypes = [vp]
    L.ocr_det_run.argtypes = [vp, C.POINTER(ocr_img), vp, C.c_int, ip, C.POINTER(C.c_double)]
    L.ocr_det_run_batch.argtypes = [vp, C.POINTER(ocr_img), C.c_int, vp, C.c_int, vp, C.POINTER(C.c_double)]
    L.ocr_det_last_shape.argtypes = [vp, ip, ip, ip]
    L.ocr_det_prob_map.argtypes = [vp, C.c_int, vp, C.c_size_t]
    L.ocr_det_bitmap.argtypes = [vp, C.c_int, vp, C.c_size_t]
    L.ocr_det_resized.argtypes = [vp, C.c_int, vp, C.c_size_t]
    L.ocr_det_post.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int, ip]
    L.ocr_det_post_stages.argtypes = [vp, C.POINTER(ocr_post_stages)]
    L.ocr_cls_cfg_default.argtypes = [C.POINTER(ocr_cls_cfg)]
    L.ocr_cls_create.argtypes = [C.POINTER(ocr_cls_cfg), C.POINTER(vp)]
    L.ocr_cls_destroy.argtypes = [vp]
    L.ocr_cls_run.argtypes = [vp, C.POINTER(ocr_img), C.c_int, vp, vp, C.POINTER(C.c_double)]
    L.ocr_cls_probs.argtypes = [vp, vp, C.c_size_t]
    L.ocr_rec_cfg_default.argtypes = [C.POINTER(ocr_rec_cfg)]
    L.ocr_rec_create.argtypes = [C.POINTER(ocr_rec_cfg), C.POINTER(vp)]
    L.ocr_rec_destroy.argtypes = [vp]
    L.ocr_rec_run.argtypes = [vp, C.POINTER(ocr_img), C.c_int, vp, C.c_int, vp, vp, C.POINTER(C.c_double)]
    L.ocr_rec_label.argtypes = [vp, C.c_int]
    L.ocr_rec_label.restype = C.c_char_p
    L.ocr_rec_num_classes.argtypes = [vp]
    L.ocr_rec_steps.argtypes = [vp, C.c_int, vp, vp, C.c_int, ip]
    L.ocr_rec_run_chars.argtypes = [vp, C.POINTER(ocr_img), C.c_int, vp, C.c_int, vp, vp, vp, vp, vp, vp, C.c_int, vp, vp,
                                    C.POINTER(C.c_double)]
    L.ocr_rec_logits_row.argtypes = [vp, C.c_int, C.c_int, vp, C.c_size_t]
    L.ocr_rec_set_launch_lines.argtypes = [vp, C.c_int]
    L.ocr_rec_timing.argtypes = [vp, C.c_int]
    L.ocr_rec_timing_report.argtypes = [vp, C.c_char_p, C.c_size_t]
    L._stage_protos_done = True


class Det:
    """DBDetector over the C-ABI (ocr_det_*).  Defaults = the literals OCRWorker passes."""

    def __init__(self, model_dir=None, device=0, limit_type="max", limit_side_len=512, thresh=0.2, box_thresh=0.4,
                 unclip_ratio=1.8, score_mode="fast", use_dilation=False, precision="fp32", max_batch=1, cv_compat=0):
        L = lib()
        _stage_protos(L)
        cfg = ocr_det_cfg()
        L.ocr_det_cfg_default(C.byref(cfg))
        self._keep = [(model_dir or os.path.join(MODELS, "det")).encode(), limit_type.encode(), score_mode.encode(),
                      precision.encode()]
        cfg.model_dir, cfg.limit_type, cfg.det_db_score_mode, cfg.precision = self._keep
        cfg.device_id, cfg.limit_side_len = device, limit_side_len
        cfg.det_db_thresh, cfg.det_db_box_thresh, cfg.det_db_unclip_ratio = thresh, box_thresh, unclip_ratio
        cfg.use_dilation, cfg.max_batch = int(use_dilation), max_batch
        cfg.cv_compat = int(cv_compat)
        self.h = C.c_void_p()
        check(L.ocr_det_create(C.byref(cfg), C.byref(self.h)))
        self.times = (C.c_double * 3)()

    def run(self, img, cap=2000):
        return self.run_batch([img], cap)[0]

    def run_batch(self, imgs, cap=2000):
        n = len(imgs)
        boxes = np.zeros((n, cap, 8), np.int32)
        cnt = np.zeros(n, np.int32)
        arr = _imgs(imgs)
        check(lib().ocr_det_run_batch(self.h, arr, n, boxes.ctypes.data, cap, cnt.ctypes.data, self.times))
        return [boxes[i, :cnt[i]].reshape(-1, 4, 2).copy() for i in range(n)]

    def last_shape(self):
        a, b, c = C.c_int(), C.c_int(), C.c_int()
        check(lib().ocr_det_last_shape(self.h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def prob_map(self, index=0):
        _, h, w = self.last_shape()
        out = np.empty((h, w), np.float32)
        check(lib().ocr_det_prob_map(self.h, index, out.ctypes.data, out.size))
        return out

    def bitmap(self, index=0):
        _, h, w = self.last_shape()
        out = np.empty((h, w), np.uint8)
        check(lib().ocr_det_bitmap(self.h, index, out.ctypes.data, out.size))
        return out

    def resized(self, index=0):
        _, h, w = self.last_shape()
        out = np.empty((h, w, 3), np.uint8)
        check(lib().ocr_det_resized(self.h, index, out.ctypes.data, out.size))
        return out

    def post(self, prob, src_h, src_w, cap=2000):
        prob = np.ascontiguousarray(prob, dtype=np.float32)
        boxes = np.zeros((cap, 8), np.int32)
        n = C.c_int()
        check(lib().ocr_det_post(self.h, prob.ctypes.data, prob.shape[0], prob.shape[1], src_h, src_w,
                                 boxes.ctypes.data, cap, C.byref(n)))
        return boxes[:n.value].reshape(-1, 4, 2).copy()

    def post_stages_raw(self, cap_pixels, cap_borders, cap_verts, null=None):
        """ocr_det_post_stages with the given capacities: (return code, the struct, the arrays it points to); `null` names a
        pointer field to pass as NULL"""
        a = dict(bitmap=np.zeros(max(cap_pixels, 1), np.uint8), starts=np.zeros(max(cap_borders, 1), np.int32),
                 npts=np.zeros(max(cap_borders, 1), np.int32), voff=np.zeros(max(cap_borders, 1), np.int32),
                 verts=np.zeros((max(cap_verts, 1), 2), np.int32), cand_valid=np.zeros(max(cap_borders, 1), np.int32),
                 cand_boxes=np.zeros((max(cap_borders, 1), 8), np.int32),
                 record=np.zeros((max(cap_borders, 1), POST_REC_FLOATS), np.float32))
        s = ocr_post_stages()
        s.cap_pixels, s.cap_borders, s.cap_verts = cap_pixels, cap_borders, cap_verts
        for k, v in a.items():
            setattr(s, k, None if k == null else v.ctypes.data)
        return lib().ocr_det_post_stages(self.h, C.byref(s)), s, a

    def post_stages(self):
        """what the last post() on this handle left behind for its map (include/ocr_hip.h, ocr_det_post_stages): a dict of
        arrays cut to their counts; `verts` a list with one (npts, 2) array per kept border (None: none stored)"""
        rc, s, _ = self.post_stages_raw(0, 0, 0)
        if rc != -4:  # OCR_ERR_CAPACITY carries the sizes; everything else (an empty map included: rc 0 is impossible at 0 pixels)
            check(rc)
        rc, s, a = self.post_stages_raw(s.rows * s.cols, s.ncont, s.nverts)
        check(rc)
        nc = s.ncont
        voff, npts = a["voff"][:nc], a["npts"][:nc]
        return dict(bitmap=a["bitmap"][:s.rows * s.cols].reshape(s.rows, s.cols), ncont_all=s.ncont_all, ncont=nc,
                    starts=a["starts"][:nc], npts=npts, cand_valid=a["cand_valid"][:nc],
                    cand_boxes=a["cand_boxes"][:nc].reshape(nc, 4, 2), record=a["record"][:nc],
                    verts=[a["verts"][voff[c]:voff[c] + npts[c]].copy() if voff[c] >= 0 else None for c in range(nc)])

    def close(self):
        if self.h:
            lib().ocr_det_destroy(self.h)
            self.h = None


class Cls:
    def __init__(self, model_dir=None, device=0, cls_thresh=0.98, cls_batch_num=8, precision="fp32"):
        L = lib()
        _stage_protos(L)
        cfg = ocr_cls_cfg()
        L.ocr_cls_cfg_default(C.byref(cfg))
        self._keep = [(model_dir or os.path.join(MODELS, "cls")).encode(), precision.encode()]
        cfg.model_dir, cfg.precision = self._keep
        cfg.device_id, cfg.cls_thresh, cfg.cls_batch_num = device, cls_thresh, cls_batch_num
        self.h = C.c_void_p()
        check(L.ocr_cls_create(C.byref(cfg), C.byref(self.h)))
        self.times = (C.c_double * 3)()

    def run(self, crops):
        n = len(crops)
        labels = np.zeros(n, np.int32)
        scores = np.zeros(n, np.float32)
        if n:
            check(lib().ocr_cls_run(self.h, _imgs(crops), n, labels.ctypes.data, scores.ctypes.data, self.times))
        return labels, scores

    def probs(self, n):
        out = np.empty((n, 2), np.float32)
        check(lib().ocr_cls_probs(self.h, out.ctypes.data, out.size))
        return out

    def close(self):
        if self.h:
            lib().ocr_cls_destroy(self.h)
            self.h = None


class Rec:
    def __init__(self, model_dir=None, device=0, label_path=None, rec_batch_num=16, rec_img_h=28, rec_img_w=192,
                 precision="fp32", sort_mode=0):
        L = lib()
        _stage_protos(L)
        cfg = ocr_rec_cfg()
        L.ocr_rec_cfg_default(C.byref(cfg))
        md = model_dir or os.path.join(MODELS, "rec")
        self._keep = [md.encode(), (label_path or os.path.join(md, "ppocr_keys_v1.txt")).encode(), precision.encode()]
        cfg.model_dir, cfg.label_path, cfg.precision = self._keep
        cfg.device_id, cfg.rec_batch_num, cfg.rec_img_h, cfg.rec_img_w = device, rec_batch_num, rec_img_h, rec_img_w
        cfg.sort_mode = int(sort_mode)
        self.h = C.c_void_p()
        check(L.ocr_rec_create(C.byref(cfg), C.byref(self.h)))
        self.times = (C.c_double * 3)()

    def run(self, crops, max_len=512):
        n = len(crops)
        ids = np.zeros((n, max_len), np.int32)
        lens = np.zeros(n, np.int32)
        scores = np.zeros(n, np.float32)
        if n:
            check(lib().ocr_rec_run(self.h, _imgs(crops), n, ids.ctypes.data, max_len, lens.ctypes.data,
                                    scores.ctypes.data, self.times))
        return [ids[i, :lens[i]].copy() for i in range(n)], scores

    def run_chars(self, crops, max_len=512, topk=0):
        """ocr_rec_run_chars: run() plus, per line, dict(steps, nsteps, probs [len], geom (T, tensor_w, resize_w) and, with
        topk > 0, alt_ids / alt_probs [len, topk]) -> (ids list, scores, chars list)"""
        n = len(crops)
        ids = np.zeros((n, max_len), np.int32)
        lens = np.zeros(n, np.int32)
        scores = np.zeros(n, np.float32)
        steps = np.zeros((n, max_len), np.int32)
        nsteps = np.zeros((n, max_len), np.int32)
        probs = np.zeros((n, max_len), np.float32)
        geom = np.zeros((n, 3), np.int32)
        kk = max(int(topk), 1)
        alt_ids = np.zeros((n, max_len, kk), np.int32)
        alt_probs = np.zeros((n, max_len, kk), np.float32)
        if n:
            check(lib().ocr_rec_run_chars(self.h, _imgs(crops), n, ids.ctypes.data, max_len, lens.ctypes.data, scores.ctypes.data,
                                          steps.ctypes.data, nsteps.ctypes.data, probs.ctypes.data, geom.ctypes.data, int(topk),
                                          alt_ids.ctypes.data, alt_probs.ctypes.data, self.times))
        chars = []
        for i in range(n):
            m = lens[i]
            c = dict(steps=steps[i, :m].copy(), nsteps=nsteps[i, :m].copy(), probs=probs[i, :m].copy(), geom=tuple(int(v) for v in geom[i]))
            if topk > 0:
                c["alt_ids"] = alt_ids[i, :m].copy()
                c["alt_probs"] = alt_probs[i, :m].copy()
            chars.append(c)
        return [ids[i, :lens[i]].copy() for i in range(n)], scores, chars

    def logits_row(self, index, step):
        """tap: the logits row the top-k kernel read for step `step` of line `index` of the last run_chars(topk > 0)"""
        out = np.zeros(self.num_classes(), np.float32)
        check(lib().ocr_rec_logits_row(self.h, int(index), int(step), out.ctypes.data, out.size))
        return out

    def steps(self, index, cap=4096):
        amax = np.zeros(cap, np.int32)
        pmax = np.zeros(cap, np.float32)
        T = C.c_int()
        check(lib().ocr_rec_steps(self.h, index, amax.ctypes.data, pmax.ctypes.data, cap, C.byref(T)))
        return amax[:T.value].copy(), pmax[:T.value].copy()

    def set_launch_lines(self, n):
        """self-test: at most n lines per network launch from the next run on (n < 1: OcrError, the handle keeps its value)"""
        check(lib().ocr_rec_set_launch_lines(self.h, int(n)))

    def timing(self, on=True):
        check(lib().ocr_rec_timing(self.h, int(on)))

    def timing_report(self):
        """{launch name: dict(ms, count, flops, bytes)} since timing(True); a name carries the shape the launch was bound to"""
        buf = C.create_string_buffer(1 << 20)
        check(lib().ocr_rec_timing_report(self.h, buf, len(buf)))
        out = {}
        for line in buf.value.decode().splitlines():
            name, ms, cnt, fl, by = line.split()
            out[name] = dict(ms=float(ms), count=int(cnt), flops=float(fl), bytes=float(by))
        return out

    def label(self, i):
        s = lib().ocr_rec_label(self.h, int(i))
        return s.decode("utf-8") if s is not None else None

    def text(self, ids):
        return "".join(self.label(i) for i in ids)

    def num_classes(self):
        return lib().ocr_rec_num_classes(self.h)

    def close(self):
        if self.h:
            lib().ocr_rec_destroy(self.h)
            self.h = None


# ---------------------------------------------------------------------------------------------
# fused pipeline + device helpers
# ---------------------------------------------------------------------------------------------
class ocr_pipe_cfg(C.Structure):
    _fields_ = [("det", ocr_det_cfg), ("cls", ocr_cls_cfg), ("rec", ocr_rec_cfg), ("enable_cls", C.c_int),
                ("crop_mode", C.c_int), ("phases", C.c_int)]


class ocr_word(C.Structure):
    _fields_ = [("box", C.c_int32 * 8), ("ids_off", C.c_int32), ("ids_len", C.c_int32), ("confidence", C.c_float)]


class ocr_char(C.Structure):
    _fields_ = [("step", C.c_int32), ("nsteps", C.c_int32), ("prob", C.c_float), ("quad", C.c_int32 * 8)]


EXPORTS += ["ocr_pipe_cfg_default", "ocr_pipe_create", "ocr_pipe_destroy", "ocr_pipe_run", "ocr_pipe_run_chars", "ocr_pipe_run_device",
            "ocr_pipe_stage", "ocr_pipe_slot_probs", "ocr_pipe_run_staged", "ocr_pipe_run_device_on", "ocr_pipe_run_staged_on", "ocr_pipe_stage_jpeg", "ocr_jpeg_decode", "ocr_jpeg_time",
            "ocr_pipe_stage_jpeg_frames", "ocr_jpeg_decode_frame", "ocr_jpeg_time_frame", "ocr_pipe_slot_image",
            "ocr_png_decode", "ocr_png_time", "ocr_png_time_batch", "ocr_pipe_stage_coded",
            "ocr_raw_decode", "ocr_raw_time", "ocr_raw_time_batch", "ocr_pipe_stage_frames",
            "ocr_tiff_decode", "ocr_tiff_time", "ocr_tiff_time_batch", "ocr_pipe_stage_batch",
            "ocr_webp_decode", "ocr_webp_time", "ocr_webp_time_batch", "ocr_vp8_decode", "ocr_vp8_time", "ocr_vp8_time_batch", "ocr_j2k_decode", "ocr_j2k_time", "ocr_j2k_time_batch",
            "ocr_j2k_tier1", "ocr_j2k_decode_coded", "ocr_j2k_time_coded", "ocr_j2k_time_coded_batch",
            "ocr_tiff_expand", "ocr_tiff_decode_coded", "ocr_tiff_time_coded", "ocr_tiff_time_coded_batch",
            "ocr_tiff_inflate", "ocr_tiff_decode_deflate", "ocr_tiff_time_deflate", "ocr_tiff_time_deflate_batch",
            "ocr_tiff_unfax", "ocr_tiff_decode_fax", "ocr_tiff_time_fax", "ocr_tiff_time_fax_batch",
            "ocr_pipe_label", "ocr_pipe_det_shape", "ocr_pipe_stats", "ocr_pipe_timing", "ocr_pipe_timing_filter", "ocr_pipe_timing_report", "ocr_dev_alloc",
            "ocr_dev_free", "ocr_dev_upload", "ocr_dev_download", "ocr_dev_sync", "ocr_dev_copy_time", "ocr_rotate_crop", "ocr_rotate_crop_shape", "ocr_rotate180_rois"]


def _pipe_protos(L):
    if getattr(L, "_pipe_protos_done", False):
        return
    _stage_protos(L)
    vp, ip = C.c_void_p, C.POINTER(C.c_int)
    L.ocr_pipe_cfg_default.argtypes = [C.POINTER(ocr_pipe_cfg)]
    L.ocr_pipe_create.argtypes = [C.POINTER(ocr_pipe_cfg), C.POINTER(vp)]
    L.ocr_pipe_destroy.argtypes = [vp]
    L.ocr_pipe_run.argtypes = [vp, C.POINTER(ocr_img), C.c_int, vp, C.c_int, vp, vp, vp, C.c_int, C.POINTER(C.c_double)]
    L.ocr_pipe_run_chars.argtypes = [vp, C.POINTER(ocr_img), C.c_int, vp, C.c_int, vp, vp, vp, C.c_int, vp, C.POINTER(C.c_double)]
    L.ocr_pipe_run_device.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int, vp, vp, vp, C.c_int,
                                      C.POINTER(C.c_double)]
    L.ocr_pipe_stage.argtypes = [vp, C.c_int, C.POINTER(ocr_img), C.c_int]
    L.ocr_pipe_slot_probs.argtypes = [vp, C.c_int, vp, C.c_int]
    L.ocr_pipe_run_staged.argtypes = [vp, C.c_int, vp, C.c_int, vp, vp, vp, C.c_int, C.POINTER(C.c_double)]
    L.ocr_pipe_run_staged_on.argtypes = [vp, C.c_int, C.c_int, vp, C.c_int, vp, vp, vp, C.c_int, C.POINTER(C.c_double)]
    L.ocr_pipe_run_device_on.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int, vp, vp, vp, C.c_int,
                                         C.POINTER(C.c_double)]
    L.ocr_pipe_label.argtypes = [vp, C.c_int]
    L.ocr_pipe_label.restype = C.c_char_p
    L.ocr_pipe_det_shape.argtypes = [vp, C.c_int, C.c_int, ip, ip]
    L.ocr_pipe_timing.argtypes = [vp, C.c_int]
    L.ocr_pipe_stats.argtypes = [vp, C.POINTER(C.c_longlong)]
    L.ocr_pipe_timing_report.argtypes = [vp, C.c_char_p, C.c_size_t]
    L.ocr_pipe_timing_filter.argtypes = [vp, C.c_char_p]
    L.ocr_dev_alloc.argtypes = [C.POINTER(vp), C.c_size_t]
    L.ocr_dev_free.argtypes = [vp]
    L.ocr_dev_upload.argtypes = [vp, vp, C.c_size_t]
    L.ocr_dev_download.argtypes = [vp, vp, C.c_size_t]
    L.ocr_rotate_crop.argtypes = [vp, C.c_int, C.c_int, C.c_size_t, vp, C.c_int, vp, C.c_size_t, vp, ip, ip]
    L.ocr_rotate_crop_shape.argtypes = [C.c_int, C.c_int, vp, ip, ip]
    L.ocr_rotate180_rois.argtypes = [vp, C.c_int, C.c_int, C.c_size_t, vp, C.c_int]
    L._pipe_protos_done = True


CROP_BOUNDING_RECT, CROP_ROTATE = 0, 1


class ocr_jpeg_comp(C.Structure):
    _fields_ = [("coef", C.c_void_p), ("quant", C.c_uint16 * 64), ("bw", C.c_int), ("bh", C.c_int), ("dw", C.c_int), ("dh", C.c_int)]


class ocr_jpeg_img(C.Structure):
    _fields_ = [("rows", C.c_int), ("cols", C.c_int), ("ncomp", C.c_int), ("hmax", C.c_int), ("vmax", C.c_int), ("orientation", C.c_int),
                ("comp", ocr_jpeg_comp * 3)]


class ocr_jpeg_fcomp(C.Structure):
    _fields_ = [("coef", C.c_void_p), ("quant", C.c_uint16 * 64), ("bw", C.c_int), ("bh", C.c_int), ("dw", C.c_int), ("dh", C.c_int),
                ("h", C.c_int), ("v", C.c_int)]


class ocr_jpeg_frame(C.Structure):
    _fields_ = [("rows", C.c_int), ("cols", C.c_int), ("ncomp", C.c_int), ("orientation", C.c_int), ("color", C.c_int), ("reserved", C.c_int),
                ("comp", ocr_jpeg_fcomp * 4)]


JPEG_COLORS = ["GREY", "YCBCR", "RGB", "CMYK", "YCCK"]


class JpegFrame:
    """an ocr_jpeg_frame over Python-owned memory.  rows, cols: the stored size; color: index into JPEG_COLORS; comps: per
    component a mapping with h, v, bw, bh, dw, dh, quant (64 values, natural order) and coef (bw * bh * 64 int16, blocks row-major).
    .coefs and the fields of .c may be changed before a call (the tests' tampering)."""

    def __init__(self, rows, cols, color, orientation, comps):
        self.coefs = [np.ascontiguousarray(k["coef"], np.int16).reshape(-1).copy() for k in comps]
        c = ocr_jpeg_frame()
        c.rows, c.cols, c.ncomp, c.orientation, c.color = rows, cols, len(comps), orientation, color
        for o, k, coef in zip(c.comp, comps, self.coefs):
            o.coef = coef.ctypes.data
            o.quant[:] = [int(q) for q in np.asarray(k["quant"]).reshape(64)]
            o.bw, o.bh, o.dw, o.dh, o.h, o.v = (int(k[f]) for f in ("bw", "bh", "dw", "dh", "h", "v"))
        self.c = c

    def out_shape(self):
        return (self.c.cols, self.c.rows) if 5 <= self.c.orientation <= 8 else (self.c.rows, self.c.cols)

    def decode(self, device_id=0, fill=0, cap=None):
        """ocr_jpeg_decode_frame: the oriented BGR image; OcrError where the call refuses (err.out: the buffer as the call left
        it, pre-filled with `fill`).  cap: the capacity in bytes the call is told instead of the buffer's"""
        return _decode_frame("ocr_jpeg_decode_frame", self.c, *self.out_shape(), device_id, fill, cap)

    def classic(self):
        """the ocr_jpeg_img that says the same, None where that descriptor cannot hold the frame (it holds grey, and YCbCr with
        luma at 1x1, 2x1 or 2x2 over 1x1 chroma)"""
        c = self.c
        f = [(c.comp[i].h, c.comp[i].v) for i in range(c.ncomp)]
        if c.ncomp == 3 and (c.color != 1 or f[0] not in ((1, 1), (2, 1), (2, 2)) or f[1:] != [(1, 1), (1, 1)]):
            return None
        if c.ncomp not in (1, 3):
            return None
        im = ocr_jpeg_img()
        im.rows, im.cols, im.ncomp, im.orientation = c.rows, c.cols, c.ncomp, c.orientation
        im.hmax, im.vmax = f[0]
        for o, k in zip(im.comp, c.comp[:c.ncomp]):
            o.coef, o.bw, o.bh, o.dw, o.dh = k.coef, k.bw, k.bh, k.dw, k.dh
            C.memmove(o.quant, k.quant, 128)
        return im

    def decode_classic(self, device_id=0, fill=0):
        """ocr_jpeg_decode of classic(): the oriented BGR image, None where ocr_jpeg_img cannot hold the frame"""
        im = self.classic()
        return None if im is None else _decode_frame("ocr_jpeg_decode", im, *self.out_shape(), device_id, fill)


class ocr_png_segment(C.Structure):
    _fields_ = [("pass_", C.c_int32), ("first_row", C.c_int32), ("rows", C.c_int32)]


class ocr_png_frame(C.Structure):
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("bit_depth", C.c_int), ("color_type", C.c_int), ("interlace", C.c_int),
                ("reserved", C.c_int), ("palette", C.c_uint8 * 768), ("data", C.c_void_p), ("data_len", C.c_size_t),
                ("segments", C.POINTER(ocr_png_segment)), ("nsegments", C.c_int)]


class PngFrame:
    """an ocr_png_frame over Python-owned memory.  stream: the inflated scanline stream (bytes); segments: [(pass, first
    row, rows)]; palette: (n, 3) RGB or None.  Fields of .c may be changed before a call (the tests' tampering)."""

    def __init__(self, width, height, bit_depth, color_type, interlace, stream, segments, palette=None):
        self._data = np.frombuffer(bytes(stream), np.uint8).copy()
        self._segs = (ocr_png_segment * max(1, len(segments)))(*[ocr_png_segment(*s) for s in segments])
        c = ocr_png_frame()
        c.width, c.height, c.bit_depth, c.color_type, c.interlace = width, height, bit_depth, color_type, interlace
        if palette is not None:
            flat = np.asarray(palette, np.uint8).reshape(-1)
            C.memmove(c.palette, flat.ctypes.data, len(flat))
        c.data, c.data_len = self._data.ctypes.data, len(self._data)
        c.segments, c.nsegments = self._segs, len(segments)
        self.c = c

    def decode(self, device_id=0):
        """ocr_png_decode: the (height, width, 3) BGR image; OcrError where the call refuses"""
        return _decode_frame("ocr_png_decode", self.c, self.c.height, self.c.width, device_id)


class ocr_raw_frame(C.Structure):
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("kind", C.c_int), ("bottom_up", C.c_int), ("row_stride", C.c_size_t),
                ("palette", C.c_uint8 * 1024), ("data", C.c_void_p), ("data_len", C.c_size_t)]


RAW_KINDS = ["INDEX1", "INDEX4", "INDEX8", "BGR555", "BGR565", "BGR24", "BGRX32", "RGB24", "GREY8", "GREY16BE", "RGB48BE", "BIT1_INV"]


class RawFrame:
    """an ocr_raw_frame over Python-owned memory.  kind: index into RAW_KINDS; rows: the stored rows (bytes or uint8 array,
    row_stride apart); palette: (n, 4) B,G,R,x or None.  Fields of .c may be changed before a call (the tests' tampering)."""

    def __init__(self, width, height, kind, bottom_up, row_stride, rows, palette=None):
        self._data = np.frombuffer(bytes(rows), np.uint8).copy() if not isinstance(rows, np.ndarray) else np.ascontiguousarray(rows, np.uint8).reshape(-1).copy()
        c = ocr_raw_frame()
        c.width, c.height, c.kind, c.bottom_up, c.row_stride = width, height, kind, bottom_up, row_stride
        if palette is not None:
            flat = np.ascontiguousarray(palette, np.uint8).reshape(-1)
            C.memmove(c.palette, flat.ctypes.data, min(1024, len(flat)))
        c.data, c.data_len = self._data.ctypes.data, len(self._data)
        self.c = c

    def decode(self, device_id=0):
        """ocr_raw_decode: the (height, width, 3) BGR image; OcrError where the call refuses"""
        return _decode_frame("ocr_raw_decode", self.c, self.c.height, self.c.width, device_id)


class ocr_tiff_frame(C.Structure):
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("photometric", C.c_int), ("bits_per_sample", C.c_int), ("samples_per_pixel", C.c_int),
                ("planar", C.c_int), ("predictor", C.c_int), ("big_endian", C.c_int), ("premultiply", C.c_int), ("tile_width", C.c_int),
                ("tile_height", C.c_int), ("palette", C.c_uint8 * 1024), ("data", C.c_void_p), ("data_len", C.c_size_t)]


class ocr_coded_frame(C.Structure):
    _fields_ = [("kind", C.c_int), ("frame", C.c_void_p)]


FRAME_JPEG, FRAME_PNG, FRAME_RAW, FRAME_TIFF, FRAME_WEBP, FRAME_VP8, FRAME_J2K, FRAME_J2K_CODED, FRAME_TIFF_CODED = 0, 1, 2, 3, 4, 5, 6, 7, 8
FRAME_TIFF_DEFLATE = 9
FRAME_TIFF_FAX = 10


def _fill_tiff_frame(f, width, height, photometric, bits, samples, tile, planar, predictor, big_endian, premultiply, palette):
    """the fields of an ocr_tiff_frame but its data"""
    f.width, f.height, f.photometric, f.bits_per_sample, f.samples_per_pixel = width, height, photometric, bits, samples
    f.planar, f.predictor, f.big_endian, f.premultiply = planar, predictor, int(big_endian), premultiply
    f.tile_width, f.tile_height = tile if tile else (width, height)
    if palette is not None:
        flat = np.ascontiguousarray(palette, np.uint8).reshape(-1)
        C.memmove(f.palette, flat.ctypes.data, min(1024, len(flat)))


def _tiff_expansion_alone(name, coded, device_id, fill, counts=False):
    """ocr_tiff_expand / ocr_tiff_inflate / ocr_tiff_unfax of a TiffCoded or TiffFax: the chunks as tiff::parse fills Frame::data
    (uint8 array, pre-filled with `fill`) - with counts (ocr_tiff_inflate): and the bytes each chunk's stream gave; OcrError
    where the call refuses (err.out: the buffer as the call left it)"""
    L = lib()
    fn = getattr(L, name)
    fn.argtypes = [C.POINTER(type(coded.c)), C.c_int, C.c_void_p, C.c_size_t] + ([C.c_void_p] if counts else [])
    n = coded.nominal()
    out = np.full(n if 0 < n <= 1 << 30 else 1, fill, np.uint8)
    produced = np.zeros(max(1, len(coded.chunks)), np.uint32)
    rc = fn(C.byref(coded.c), device_id, out.ctypes.data, out.size, *([produced.ctypes.data] if counts else []))
    if rc != 0:
        _raise(L, rc, out)
    return (out, produced[:len(coded.chunks)]) if counts else out


class TiffFrame:
    """an ocr_tiff_frame over Python-owned memory.  chunks: the expanded chunks at their nominal size (bytes or uint8 array);
    tile: (width, height) of a chunk, None for one strip; palette: (n, 4) B,G,R,x or None.  Fields of .c may be changed before
    a call (the tests' tampering; bits -> bits_per_sample, samples -> samples_per_pixel, w / h -> width / height)."""

    def __init__(self, width, height, photometric, bits, samples, chunks, tile=None, planar=1, predictor=1, big_endian=0, premultiply=0, palette=None):
        self._data = np.frombuffer(bytes(chunks), np.uint8).copy() if not isinstance(chunks, np.ndarray) else np.ascontiguousarray(chunks, np.uint8).reshape(-1).copy()
        c = ocr_tiff_frame()
        _fill_tiff_frame(c, width, height, photometric, bits, samples, tile, planar, predictor, big_endian, premultiply, palette)
        c.data, c.data_len = self._data.ctypes.data, len(self._data)
        self.c = c

    def decode(self, device_id=0):
        """ocr_tiff_decode: the (height, width, 3) BGR image; OcrError where the call refuses"""
        return _decode_frame("ocr_tiff_decode", self.c, self.c.height, self.c.width, device_id)


class ocr_tiff_coded(C.Structure):
    _fields_ = [("frame", ocr_tiff_frame), ("compression", C.c_int), ("chunks", C.c_void_p), ("chunks_len", C.c_size_t), ("bytes", C.c_void_p),
                ("bytes_len", C.c_size_t)]


# ocr_tiff_chunk as a numpy record (16 bytes)
TIFF_CHUNK = np.dtype([("byte_off", "<u8"), ("byte_len", "<u4"), ("rows", "<u4")])


class TiffCoded:
    """an ocr_tiff_coded over Python-owned memory: the frame before its chunks are expanded.  compression: 1, 5 or 32773;
    chunks: the records (TIFF_CHUNK: byte_off, byte_len, rows) in the order of the expanded chunks; data: the byte pool; the
    rest as for TiffFrame.  .chunks / .data and the fields of .c may be changed before a call (the tests' tampering)."""

    def __init__(self, width, height, photometric, bits, samples, compression, chunks, data, tile=None, planar=1, predictor=1, big_endian=0, premultiply=0,
                 palette=None):
        self.chunks = np.array(chunks, TIFF_CHUNK).reshape(-1)
        self.data = np.frombuffer(bytes(data), np.uint8).copy() if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, np.uint8).reshape(-1).copy()
        c = ocr_tiff_coded()
        _fill_tiff_frame(c.frame, width, height, photometric, bits, samples, tile, planar, predictor, big_endian, premultiply, palette)
        c.frame.data, c.frame.data_len = None, 0
        c.compression = compression
        c.chunks, c.chunks_len = self.chunks.ctypes.data if len(self.chunks) else None, len(self.chunks)
        c.bytes, c.bytes_len = self.data.ctypes.data if len(self.data) else None, len(self.data)
        self.c = c

    def nominal(self):
        """the bytes of the expanded chunks at their nominal size (0 where the geometry is out of range)"""
        f = self.c.frame
        if min(f.width, f.height, f.tile_width, f.tile_height, f.bits_per_sample, f.samples_per_pixel) <= 0:
            return 0
        planes = f.samples_per_pixel if f.planar == 2 else 1
        row = (f.tile_width * (1 if f.planar == 2 else f.samples_per_pixel) * f.bits_per_sample + 7) // 8
        return row * f.tile_height * (-(-f.width // f.tile_width)) * (-(-f.height // f.tile_height)) * planes

    def expand(self, device_id=0, fill=0):
        """ocr_tiff_expand: the chunks as tiff::parse fills Frame::data (uint8 array); OcrError where the call refuses"""
        return _tiff_expansion_alone("ocr_tiff_expand", self, device_id, fill)

    def decode(self, device_id=0, fill=0):
        """ocr_tiff_decode_coded: the (height, width, 3) BGR image; OcrError where the call refuses (err.out: the buffer as the
        call left it, pre-filled with `fill`)"""
        return _decode_frame("ocr_tiff_decode_coded", self.c, self.c.frame.height, self.c.frame.width, device_id, fill)

    def time(self, iters=3, device_id=0):
        """ocr_tiff_time_coded: [upload, expansion, pixel stage] in ms"""
        return time_tiff_coded([self], iters, device_id, single=True)

    # the Deflate route (compression 8 or 32946)
    def inflate(self, device_id=0, fill=0):
        """ocr_tiff_inflate: (the chunks as tiff::parse fills Frame::data, the bytes each chunk's stream gave); OcrError where
        the call refuses (err.out: the buffer as the call left it, pre-filled with `fill`)"""
        return _tiff_expansion_alone("ocr_tiff_inflate", self, device_id, fill, counts=True)

    def decode_deflate(self, device_id=0, fill=0):
        """ocr_tiff_decode_deflate: the (height, width, 3) BGR image; OcrError where the call refuses (err.out as for decode)"""
        return _decode_frame("ocr_tiff_decode_deflate", self.c, self.c.frame.height, self.c.frame.width, device_id, fill)


def tiff_expand(coded, device_id=0):
    """ocr_tiff_expand of a TiffCoded"""
    return coded.expand(device_id)


def tiff_decode_coded(coded, device_id=0):
    """ocr_tiff_decode_coded of a TiffCoded"""
    return coded.decode(device_id)


def time_tiff_coded(coded, iters=3, device_id=0, single=False):
    """ocr_tiff_time_coded_batch over TiffCoded objects as one batch (single: ocr_tiff_time_coded of the first):
    [upload, expansion, pixel stage] in ms"""
    return _time_coded("ocr_tiff_time_coded", coded, iters, device_id, single)


def tiff_inflate(coded, device_id=0):
    """ocr_tiff_inflate of a TiffCoded with a Deflate compression: (chunks, produced)"""
    return coded.inflate(device_id)


def tiff_decode_deflate(coded, device_id=0):
    """ocr_tiff_decode_deflate of a TiffCoded with a Deflate compression"""
    return coded.decode_deflate(device_id)


def time_tiff_deflate(coded, iters=3, device_id=0, single=False):
    """ocr_tiff_time_deflate_batch over TiffCoded objects as one batch (single: ocr_tiff_time_deflate of the first):
    [upload, inflate with its read-back, pixel stage] in ms"""
    return _time_coded("ocr_tiff_time_deflate", coded, iters, device_id, single)


class ocr_tiff_fax(C.Structure):
    _fields_ = [("coded", ocr_tiff_coded), ("t4_options", C.c_uint32)]


class TiffFax:
    """an ocr_tiff_fax over Python-owned memory: a CCITT frame before its chunks are expanded.  compression: 2, 3, 4 or 32771;
    t4_options: T4Options of Compression 3; chunks and data as for TiffCoded.  The frame is 1 bit, 1 sample; the fields of
    .c.coded and .c.t4_options may be changed before a call (the tests' tampering)."""

    def __init__(self, width, height, photometric, compression, chunks, data, tile=None, t4_options=0):
        self.inner = TiffCoded(width, height, photometric, 1, 1, compression, chunks, data, tile=tile)
        self.chunks, self.data = self.inner.chunks, self.inner.data
        self.c = ocr_tiff_fax()
        C.memmove(C.byref(self.c.coded), C.byref(self.inner.c), C.sizeof(ocr_tiff_coded))
        self.c.t4_options = t4_options

    def nominal(self):
        C.memmove(C.byref(self.inner.c), C.byref(self.c.coded), C.sizeof(ocr_tiff_coded))
        return self.inner.nominal()

    def unfax(self, device_id=0, fill=0):
        """ocr_tiff_unfax: the chunks as tiff::parse fills Frame::data (uint8 array, pre-filled with `fill`); OcrError where the
        call refuses (err.out: the buffer as the call left it)"""
        return _tiff_expansion_alone("ocr_tiff_unfax", self, device_id, fill)

    def decode(self, device_id=0, fill=0):
        """ocr_tiff_decode_fax: the (height, width, 3) BGR image; OcrError where the call refuses (err.out as for unfax)"""
        return _decode_frame("ocr_tiff_decode_fax", self.c, self.c.coded.frame.height, self.c.coded.frame.width, device_id, fill)

    def time(self, iters=3, device_id=0):
        """ocr_tiff_time_fax: [upload, expansion, pixel stage] in ms"""
        return time_tiff_fax([self], iters, device_id, single=True)


def tiff_unfax(fax, device_id=0):
    """ocr_tiff_unfax of a TiffFax"""
    return fax.unfax(device_id)


def tiff_decode_fax(fax, device_id=0):
    """ocr_tiff_decode_fax of a TiffFax"""
    return fax.decode(device_id)


def time_tiff_fax(fax, iters=3, device_id=0, single=False):
    """ocr_tiff_time_fax_batch over TiffFax objects as one batch (single: ocr_tiff_time_fax of the first):
    [upload, expansion, pixel stage] in ms"""
    return _time_coded("ocr_tiff_time_fax", fax, iters, device_id, single)


class ocr_webp_transform(C.Structure):
    _fields_ = [("kind", C.c_int), ("bits", C.c_int), ("data", C.c_void_p), ("data_len", C.c_size_t)]


class ocr_webp_frame(C.Structure):
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("argb", C.c_void_p), ("argb_len", C.c_size_t), ("ntransforms", C.c_int),
                ("transforms", ocr_webp_transform * 4)]


class WebpFrame:
    """an ocr_webp_frame over Python-owned memory.  coded: the entropy-decoded image (uint32 A << 24 | R << 16 | G << 8 | B, coded
    width x height); transforms: up to four (kind, bits, data) in file order, data a uint32 array (sub-image or palette) or None.
    Fields of .c may be changed before a call (the tests' tampering)."""

    def __init__(self, width, height, coded, transforms=()):
        self._coded = np.ascontiguousarray(coded, np.uint32).reshape(-1).copy()
        self._data = []
        c = ocr_webp_frame()
        c.width, c.height = width, height
        c.argb, c.argb_len = self._coded.ctypes.data, len(self._coded)
        c.ntransforms = len(transforms)
        for k, (kind, bits, data) in enumerate(list(transforms)[:4]):
            c.transforms[k].kind, c.transforms[k].bits = kind, bits
            if data is not None:
                a = np.ascontiguousarray(data, np.uint32).reshape(-1).copy()
                self._data.append(a)
                c.transforms[k].data, c.transforms[k].data_len = a.ctypes.data, len(a)
        self.c = c

    def decode(self, device_id=0):
        """ocr_webp_decode: the (height, width, 3) BGR image; OcrError where the call refuses"""
        return _decode_frame("ocr_webp_decode", self.c, self.c.height, self.c.width, device_id)


class ocr_vp8_frame(C.Structure):
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("filter_type", C.c_int), ("mbs", C.c_void_p), ("mbs_len", C.c_size_t),
                ("coeffs", C.c_void_p), ("coeffs_len", C.c_size_t)]


# ocr_vp8_mb as a numpy record (40 bytes)
VP8_MB = np.dtype([("modes", "u1", 16), ("is_i4x4", "u1"), ("uvmode", "u1"), ("level", "u1"), ("ilevel", "u1"), ("hev", "u1"), ("inner", "u1"),
                   ("segment", "u1"), ("skip", "u1"), ("nz_y", "<u4"), ("nz_uv", "<u4"), ("present", "<u4"), ("coeff_off", "<u4")])


class Vp8Frame:
    """an ocr_vp8_frame over Python-owned memory.  mbs: the macroblock records (VP8_MB, raster order); coeffs: the int16
    coefficients of the shipped blocks.  .mbs / .coeffs and the fields of .c may be changed before a call (the tests' tampering)."""

    def __init__(self, width, height, filter_type, mbs, coeffs):
        self.mbs = np.array(mbs, VP8_MB).reshape(-1)
        self.coeffs = np.ascontiguousarray(coeffs, np.int16).reshape(-1).copy()
        c = ocr_vp8_frame()
        c.width, c.height, c.filter_type = width, height, filter_type
        c.mbs, c.mbs_len = self.mbs.ctypes.data, len(self.mbs)
        c.coeffs, c.coeffs_len = self.coeffs.ctypes.data if len(self.coeffs) else None, len(self.coeffs)
        self.c = c

    def decode(self, device_id=0, fill=0):
        """ocr_vp8_decode: the (height, width, 3) BGR image; OcrError where the call refuses (err.out: the buffer as the call left
        it, pre-filled with `fill`)"""
        return _decode_frame("ocr_vp8_decode", self.c, self.c.height, self.c.width, device_id, fill)


class ocr_j2k_frame(C.Structure):
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("x0", C.c_int), ("y0", C.c_int), ("ncomp", C.c_int), ("prec", C.c_int), ("transform", C.c_int),
                ("mct", C.c_int), ("chan", C.c_int * 3), ("tcs", C.c_void_p), ("tcs_len", C.c_size_t), ("steps", C.c_void_p), ("steps_len", C.c_size_t),
                ("coeffs", C.c_void_p), ("coeffs_len", C.c_size_t)]


# ocr_j2k_tilecomp as a numpy record (40 bytes)
J2K_TC = np.dtype([("x0", "<i4"), ("y0", "<i4"), ("x1", "<i4"), ("y1", "<i4"), ("levels", "<i4"), ("comp", "<i4"), ("step_off", "<u4"), ("reserved", "<u4"),
                   ("coeff_off", "<u8")])


class J2kFrame:
    """an ocr_j2k_frame over Python-owned memory.  tcs: the tile-component records (J2K_TC, ncomp a tile, tiles in raster order);
    steps: float32 step sizes; coeffs: int32 coefficients in the band arrangement.  .tcs / .steps / .coeffs and the fields of
    .c may be changed before a call (the tests' tampering)."""

    def __init__(self, width, height, x0, y0, ncomp, prec, transform, mct, chan, tcs, steps, coeffs):
        self.tcs = np.array(tcs, J2K_TC).reshape(-1)
        self.steps = np.ascontiguousarray(steps, np.float32).reshape(-1).copy()
        self.coeffs = np.ascontiguousarray(coeffs, np.int32).reshape(-1).copy()
        c = ocr_j2k_frame()
        c.width, c.height, c.x0, c.y0, c.ncomp, c.prec, c.transform, c.mct = width, height, x0, y0, ncomp, prec, transform, mct
        c.chan[0], c.chan[1], c.chan[2] = chan
        c.tcs, c.tcs_len = self.tcs.ctypes.data, len(self.tcs)
        c.steps, c.steps_len = self.steps.ctypes.data, len(self.steps)
        c.coeffs, c.coeffs_len = self.coeffs.ctypes.data, len(self.coeffs)
        self.c = c

    def decode(self, device_id=0, fill=0):
        """ocr_j2k_decode: the (height, width, 3) BGR image; OcrError where the call refuses (err.out: the buffer as the call left
        it, pre-filled with `fill`)"""
        return _decode_frame("ocr_j2k_decode", self.c, self.c.height, self.c.width, device_id, fill)


class ocr_j2k_coded(C.Structure):
    _fields_ = [("frame", ocr_j2k_frame), ("cblks", C.c_void_p), ("cblks_len", C.c_size_t), ("bytes", C.c_void_p), ("bytes_len", C.c_size_t)]


# ocr_j2k_cblk as a numpy record (32 bytes)
J2K_CBLK = np.dtype([("tc", "<u4"), ("at", "<u4"), ("byte_off", "<u8"), ("byte_len", "<u4"), ("w", "<u2"), ("h", "<u2"), ("orient", "u1"), ("numbps", "u1"),
                     ("passes", "u1"), ("reserved", "u1"), ("reserved2", "<u4")])


class J2kCoded:
    """an ocr_j2k_coded over Python-owned memory: the frame before tier-1.  tcs, steps as for J2kFrame; ncoeffs: the size of the
    coefficient plane; cblks: the code-block records (J2K_CBLK); data: the blocks' bytes.  .tcs / .steps / .cblks / .data and
    the fields of .c may be changed before a call (the tests' tampering)."""

    def __init__(self, width, height, x0, y0, ncomp, prec, transform, mct, chan, tcs, steps, ncoeffs, cblks, data):
        self.tcs = np.array(tcs, J2K_TC).reshape(-1)
        self.steps = np.ascontiguousarray(steps, np.float32).reshape(-1).copy()
        self.cblks = np.array(cblks, J2K_CBLK).reshape(-1)
        self.data = np.frombuffer(bytes(data), np.uint8).copy() if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, np.uint8).reshape(-1).copy()
        c = ocr_j2k_coded()
        f = c.frame
        f.width, f.height, f.x0, f.y0, f.ncomp, f.prec, f.transform, f.mct = width, height, x0, y0, ncomp, prec, transform, mct
        f.chan[0], f.chan[1], f.chan[2] = chan
        f.tcs, f.tcs_len = self.tcs.ctypes.data, len(self.tcs)
        f.steps, f.steps_len = self.steps.ctypes.data, len(self.steps)
        f.coeffs, f.coeffs_len = None, int(ncoeffs)
        c.cblks, c.cblks_len = self.cblks.ctypes.data if len(self.cblks) else None, len(self.cblks)
        c.bytes, c.bytes_len = self.data.ctypes.data if len(self.data) else None, len(self.data)
        self.c = c

    def tier1(self, device_id=0, fill=0):
        """ocr_j2k_tier1: the int32 coefficient plane; OcrError where the call refuses (err.out: the buffer as the call left it)"""
        L = lib()
        L.ocr_j2k_tier1.argtypes = [C.POINTER(ocr_j2k_coded), C.c_int, C.c_void_p, C.c_size_t]
        n = self.c.frame.coeffs_len
        out = np.full(n if 0 < n <= 1 << 28 else 1, fill, np.int32)
        rc = L.ocr_j2k_tier1(C.byref(self.c), device_id, out.ctypes.data, out.size)
        if rc != 0:
            _raise(L, rc, out)
        return out

    def decode(self, device_id=0, fill=0):
        """ocr_j2k_decode_coded: the (height, width, 3) BGR image; OcrError where the call refuses (err.out: the buffer as the
        call left it, pre-filled with `fill`)"""
        return _decode_frame("ocr_j2k_decode_coded", self.c, self.c.frame.height, self.c.frame.width, device_id, fill)

    def time(self, iters=3, device_id=0):
        """ocr_j2k_time_coded: [upload, tier-1, pixel stage] in ms"""
        return time_j2k_coded([self], iters, device_id, single=True)


def time_j2k_coded(coded, iters=3, device_id=0, single=False):
    """ocr_j2k_time_coded_batch over J2kCoded objects as one batch (single: ocr_j2k_time_coded of the first):
    [upload, tier-1, pixel stage] in ms"""
    return _time_coded("ocr_j2k_time_coded", coded, iters, device_id, single)


def rotate_crop_shape(rows, cols, box):
    """ocr_rotate_crop_shape: (rows, cols) of GetRotateCropImage's result (host arithmetic only)."""
    L = lib()
    _pipe_protos(L)
    b = np.ascontiguousarray(np.asarray(box, np.int32).reshape(8))
    r, c = C.c_int(), C.c_int()
    check(L.ocr_rotate_crop_shape(rows, cols, b.ctypes.data, C.byref(r), C.byref(c)))
    return r.value, c.value


def rotate180_rois(img, rects):
    """ocr_rotate180_rois: in-place 180-degree rotation of the (x, y, w, h) rectangles of a BGR u8 image, in list order."""
    L = lib()
    _pipe_protos(L)
    img = np.ascontiguousarray(img, dtype=np.uint8).copy()
    r = np.ascontiguousarray(rects, dtype=np.int32).reshape(-1, 4)
    check(L.ocr_rotate180_rois(img.ctypes.data, img.shape[0], img.shape[1], img.strides[0], r.ctypes.data, len(r)))
    return img


def rotate_crops(img, boxes):
    """Utility::GetRotateCropImage for each box of one image on the device (ocr_rotate_crop)."""
    L = lib()
    _pipe_protos(L)
    img = np.asarray(img, np.uint8)
    assert img.ndim == 3 and img.shape[2] == 3 and img.strides[1] == 3 and img.strides[2] == 1
    b = np.ascontiguousarray(np.asarray(boxes, np.int32).reshape(-1, 8))
    n = b.shape[0]
    shapes = [rotate_crop_shape(img.shape[0], img.shape[1], b[k]) for k in range(n)]
    cap = sum(r * c * 3 for r, c in shapes)
    out = np.empty(max(cap, 1), np.uint8)
    off = np.zeros(n + 1, np.uint64)
    rr, cc = (C.c_int * n)(), (C.c_int * n)()
    check(L.ocr_rotate_crop(img.ctypes.data, img.shape[0], img.shape[1], img.strides[0], b.ctypes.data, n, out.ctypes.data,
                            cap, off.ctypes.data, rr, cc))
    return [out[int(off[k]):int(off[k + 1])].reshape(rr[k], cc[k], 3).copy() for k in range(n)]


class DevArray:
    """A device allocation filled from a numpy array (inputs 'already resident in HBM')."""

    def __init__(self, host):
        L = lib()
        _pipe_protos(L)
        host = np.ascontiguousarray(host)
        self.nbytes = host.nbytes
        self.shape, self.dtype = host.shape, host.dtype
        self.ptr = C.c_void_p()
        check(L.ocr_dev_alloc(C.byref(self.ptr), self.nbytes))
        check(L.ocr_dev_upload(self.ptr, host.ctypes.data, self.nbytes))

    def download(self):
        out = np.empty(self.shape, self.dtype)
        check(lib().ocr_dev_download(out.ctypes.data, self.ptr, self.nbytes))
        return out

    def free(self):
        if self.ptr:
            lib().ocr_dev_free(self.ptr)
            self.ptr = None


class Pipe:
    """OCRWorker::processRequest over the C-ABI (ocr_pipe_*) for batches of images."""

    def __init__(self, model_root=None, device=0, enable_cls=False, limit_type="max", limit_side_len=512, thresh=0.2,
                 box_thresh=0.4, unclip_ratio=1.8, use_dilation=False, rec_batch_num=16, rec_img_h=28, rec_img_w=192,
                 cls_batch_num=8, crop_mode=CROP_BOUNDING_RECT, score_mode="fast", rec_sort_mode=0, phases=0, cv_compat=0,
                 precision="fp32", det_dir=None, rec_dir=None):
        """det_dir / rec_dir: model directories of their own (BASELINE configs[4]: models_server/det, models_server/rec -
        directories whose arch.txt names a server plan); the dictionary stays the reference's"""
        L = lib()
        _pipe_protos(L)
        root = model_root or MODELS
        cfg = ocr_pipe_cfg()
        L.ocr_pipe_cfg_default(C.byref(cfg))
        self._keep = [(det_dir or os.path.join(root, "det")).encode(), os.path.join(root, "cls").encode(),
                      (rec_dir or os.path.join(root, "rec")).encode(), os.path.join(root, "rec", "ppocr_keys_v1.txt").encode(),
                      limit_type.encode(), score_mode.encode(), precision.encode()]
        (cfg.det.model_dir, cfg.cls.model_dir, cfg.rec.model_dir, cfg.rec.label_path, cfg.det.limit_type,
         cfg.det.det_db_score_mode, _prec) = self._keep
        cfg.det.precision = cfg.cls.precision = cfg.rec.precision = _prec
        cfg.det.device_id = device
        cfg.det.limit_side_len = limit_side_len
        cfg.det.det_db_thresh, cfg.det.det_db_box_thresh, cfg.det.det_db_unclip_ratio = thresh, box_thresh, unclip_ratio
        cfg.det.use_dilation = int(use_dilation)
        cfg.det.cv_compat = int(cv_compat)
        cfg.rec.rec_batch_num, cfg.rec.rec_img_h, cfg.rec.rec_img_w = rec_batch_num, rec_img_h, rec_img_w
        cfg.rec.sort_mode = int(rec_sort_mode)
        cfg.cls.cls_batch_num = cls_batch_num
        cfg.enable_cls = int(enable_cls)
        cfg.crop_mode = int(crop_mode)
        cfg.phases = int(phases)
        self.h = C.c_void_p()
        check(L.ocr_pipe_create(C.byref(cfg), C.byref(self.h)))
        self.times = (C.c_double * 3)()
        self._cap_words, self._cap_ids = 0, 0

    def _bufs(self, count):
        cw, ci = count * 1000, count * 1000 * 64
        if cw > self._cap_words:
            self._words = (ocr_word * cw)()
            self._ids = np.zeros(ci, np.int32)
            self._cap_words, self._cap_ids = cw, ci
        return self._words, self._ids

    def _collect(self, count, words, ids, off, nw):
        out = []
        for i in range(count):
            ws = []
            for k in range(off[i], off[i] + nw[i]):
                w = words[k]
                ws.append(dict(box=np.array(w.box[:], np.int32).reshape(4, 2),
                               ids=ids[w.ids_off:w.ids_off + w.ids_len].copy(), confidence=float(w.confidence)))
            out.append(ws)
        return out

    def run(self, imgs):
        n = len(imgs)
        words, ids = self._bufs(n)
        off = np.zeros(n, np.int32)
        nw = np.zeros(n, np.int32)
        check(lib().ocr_pipe_run(self.h, _imgs(imgs), n, words, self._cap_words, off.ctypes.data, nw.ctypes.data,
                                 ids.ctypes.data, self._cap_ids, self.times))
        return self._collect(n, words, ids, off, nw)

    def run_chars(self, imgs):
        """ocr_pipe_run_chars: run() with, per word, chars = [dict(step, nsteps, prob, quad [4, 2])] parallel to its ids"""
        n = len(imgs)
        words, ids = self._bufs(n)
        chars = np.zeros((self._cap_ids, 11), np.int32)  # ocr_char: 11 dwords (step, nsteps, prob as f32 bits, quad[8])
        assert C.sizeof(ocr_char) == 44
        off = np.zeros(n, np.int32)
        nw = np.zeros(n, np.int32)
        check(lib().ocr_pipe_run_chars(self.h, _imgs(imgs), n, words, self._cap_words, off.ctypes.data, nw.ctypes.data,
                                       ids.ctypes.data, self._cap_ids, chars.ctypes.data, self.times))
        out = self._collect(n, words, ids, off, nw)
        for i in range(n):
            for k, w in enumerate(out[i]):
                cw = words[off[i] + k]
                rows = chars[cw.ids_off:cw.ids_off + cw.ids_len]
                w["chars"] = [dict(step=int(r[0]), nsteps=int(r[1]), prob=float(r[2:3].view(np.float32)[0]),
                                   quad=r[3:].reshape(4, 2).copy()) for r in rows]
        return out

    def stage(self, slot, imgs, probs=None):
        """ocr_pipe_stage: host images (any sizes) -> pinned memory -> device, asynchronously.  probs: per image a
        float32 map of the detector's input resolution (det_shape), attached with ocr_pipe_slot_probs; None keeps
        whatever maps the slot has (they survive re-staging the same sizes in the same order)."""
        n = len(imgs)
        self._staged_n = getattr(self, "_staged_n", {})
        check(lib().ocr_pipe_stage(self.h, slot, _imgs(imgs), n))
        self._staged_n[slot] = n
        if probs is not None:
            arr = (C.c_void_p * n)()
            maps = [np.ascontiguousarray(p, dtype=np.float32) for p in probs]
            for i, m in enumerate(maps):
                arr[i] = m.ctypes.data
            check(lib().ocr_pipe_slot_probs(self.h, slot, arr, n))

    def stage_dev_probs(self, slot, imgs, dev_probs):
        """ocr_pipe_stage with probability maps that already sit in device memory (DevArray per image): they are copied
        device to device into the slot (a request stream's maps are uploaded once per distinct image, not per batch)."""
        n = len(imgs)
        self._staged_n = getattr(self, "_staged_n", {})
        check(lib().ocr_pipe_stage(self.h, slot, _imgs(imgs), n))
        self._staged_n[slot] = n
        arr = (C.c_void_p * n)()
        for i, d in enumerate(dev_probs):
            arr[i] = d.ptr.value
        check(lib().ocr_pipe_slot_probs(self.h, slot, arr, n))

    def stage_jpeg_frames(self, slot, frames):
        """ocr_pipe_stage_jpeg_frames: a list of JpegFrame as one batch into the slot (one IDCT launch over all their planes)"""
        L = lib()
        L.ocr_pipe_stage_jpeg_frames.argtypes = [C.c_void_p, C.c_int, C.POINTER(ocr_jpeg_frame), C.c_int]
        arr = (ocr_jpeg_frame * len(frames))(*[f.c for f in frames])  # (copies of the structs: the coefficient arrays stay the frames')
        check(L.ocr_pipe_stage_jpeg_frames(self.h, slot, arr, len(frames)))
        self._staged_n = getattr(self, "_staged_n", {})
        self._staged_n[slot] = len(frames)

    def slot_image(self, slot, index, rows, cols):
        """ocr_pipe_slot_image: the staged image that was number `index` of the slot's last stage call, (rows, cols, 3) BGR;
        rows, cols: the size the caller expects (the buffer's capacity) - the call's own answer is asserted against it"""
        L = lib()
        L.ocr_pipe_slot_image.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        out = np.zeros((rows, cols, 3), np.uint8)
        r, c = C.c_int(), C.c_int()
        check(L.ocr_pipe_slot_image(self.h, slot, index, out.ctypes.data, out.size, C.byref(r), C.byref(c)))
        assert (r.value, c.value) == (rows, cols), (r.value, c.value, rows, cols)
        return out

    def stats(self):
        """{'runs', 'binds', 'graph_replays'} summed over the pipeline's networks (Net::stats)"""
        out = (C.c_longlong * 3)()
        check(lib().ocr_pipe_stats(self.h, out))
        return dict(runs=int(out[0]), binds=int(out[1]), graph_replays=int(out[2]))

    def run_staged(self, slot, collect=True):
        count = self._staged_n[slot]
        words, ids = self._bufs(count)
        off = np.zeros(count, np.int32)
        nw = np.zeros(count, np.int32)
        check(lib().ocr_pipe_run_staged(self.h, slot, words, self._cap_words, off.ctypes.data, nw.ctypes.data, ids.ctypes.data,
                                        self._cap_ids, self.times))
        return self._collect(count, words, ids, off, nw) if collect else int(nw.sum())

    def run_device(self, dev_imgs, rows, cols, count, dev_prob=None, collect=True):
        words, ids = self._bufs(count)
        off = np.zeros(count, np.int32)
        nw = np.zeros(count, np.int32)
        check(lib().ocr_pipe_run_device(self.h, dev_imgs.ptr, rows, cols, count, dev_prob.ptr if dev_prob else None,
                                        words, self._cap_words, off.ctypes.data, nw.ctypes.data, ids.ctypes.data,
                                        self._cap_ids, self.times))
        return self._collect(count, words, ids, off, nw) if collect else int(nw.sum())

    # ---- two batches in flight (ocr_pipe_run_device_on / ocr_pipe_run_staged_on): the whole batch on one chain; calls on
    # different chains may run concurrently from different threads - result buffers and stage times are per chain
    def _chain_bufs(self, chain, count):
        if not hasattr(self, "_cb"):
            self._cb = {}
        cw, ci = count * 1000, count * 1000 * 64
        b = self._cb.get(chain)
        if b is None or b[2] < cw:
            b = self._cb[chain] = ((ocr_word * cw)(), np.zeros(ci, np.int32), cw, ci, (C.c_double * 3)())
        return b

    def run_device_on(self, chain, dev_imgs, rows, cols, count, dev_prob=None, collect=True):
        words, ids, cw, ci, times = self._chain_bufs(chain, count)
        off = np.zeros(count, np.int32)
        nw = np.zeros(count, np.int32)
        check(lib().ocr_pipe_run_device_on(self.h, chain, dev_imgs.ptr, rows, cols, count, dev_prob.ptr if dev_prob else None,
                                           words, cw, off.ctypes.data, nw.ctypes.data, ids.ctypes.data, ci, times))
        return self._collect(count, words, ids, off, nw) if collect else int(nw.sum())

    def run_staged_on(self, chain, slot, collect=True):
        count = self._staged_n[slot]
        words, ids, cw, ci, times = self._chain_bufs(chain, count)
        off = np.zeros(count, np.int32)
        nw = np.zeros(count, np.int32)
        check(lib().ocr_pipe_run_staged_on(self.h, chain, slot, words, cw, off.ctypes.data, nw.ctypes.data, ids.ctypes.data, ci, times))
        return self._collect(count, words, ids, off, nw) if collect else int(nw.sum())

    def chain_times(self, chain):
        return list(self._cb[chain][4]) if hasattr(self, "_cb") and chain in self._cb else None

    def det_shape(self, rows, cols):
        a, b = C.c_int(), C.c_int()
        check(lib().ocr_pipe_det_shape(self.h, rows, cols, C.byref(a), C.byref(b)))
        return a.value, b.value

    def label(self, i):
        s = lib().ocr_pipe_label(self.h, int(i))
        return s.decode("utf-8") if s is not None else None

    def timing(self, on=True, only=None):
        """HIP events around network launches; `only`: restrict them to launches whose name contains it."""
        check(lib().ocr_pipe_timing_filter(self.h, only.encode() if only else None))
        check(lib().ocr_pipe_timing(self.h, int(on)))

    def timing_report(self):
        buf = C.create_string_buffer(1 << 24)   # one row per (launch, bound shape): a mixed-size batch has tens of thousands
        check(lib().ocr_pipe_timing_report(self.h, buf, len(buf)))
        out = {}
        for line in buf.value.decode().splitlines():
            name, ms, cnt, fl, by = line.split()
            r = out.setdefault(name, dict(ms=0.0, count=0, flops=0.0, bytes=0.0))  # both rec lanes share names
            r["ms"] += float(ms)
            r["count"] += int(cnt)
            r["flops"] += float(fl)
            r["bytes"] += float(by)
        return out

    def close(self):
        if self.h:
            lib().ocr_pipe_destroy(self.h)
            self.h = None
