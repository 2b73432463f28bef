/* libocr_hip — C-ABI of the MI355X-native OCR hot path (det -> cls -> rec).
 *
 * Drop-in boundary: these entry points are what a maintainer of sssxyd/cpp-paddle-ocr binds in
 * place of the Paddle Inference predictor + OpenCV pre/post code inside
 *   DBDetector::Run        /root/reference/src/ocr_det.cpp:93-176   (include/paddle_ocr/ocr_det.h:95-97)
 *   Classifier::Run        /root/reference/src/ocr_cls.cpp:23-106   (include/paddle_ocr/ocr_cls.h:81-82)
 *   CRNNRecognizer::Run    /root/reference/src/ocr_rec.cpp:24-135   (include/paddle_ocr/ocr_rec.h:92-95)
 *   OCRWorker::processRequest  /root/reference/src/ocr_worker.cpp:213-311
 * Plain pointers and sizes only; every function returns 0 on success and a negative code on
 * failure (never exit(): compare ocr_det.cpp:41-45).  ocr_last_error() gives the message of the
 * calling thread's last failure.  One handle = one HIP stream + its device buffers; use one
 * handle per host thread (the reference's stage objects are not re-entrant either).
 * INTEGRATION.md shows the C++ shim classes that keep the reference signatures on top of this.
 */
#ifndef OCR_HIP_H_
#define OCR_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OCR_OK 0
#define OCR_ERR_ARG (-1)      /* bad argument */
#define OCR_ERR_MODEL (-2)    /* model files missing / do not match the supported graph */
#define OCR_ERR_DEVICE (-3)   /* HIP runtime failure (message has the HIP error string) */
#define OCR_ERR_CAPACITY (-4) /* caller buffer too small */

const char* ocr_last_error(void);
/* Selects the HIP device for the calling thread; fails when no gfx950 device is visible. */
int ocr_rt_init(int device_id);
int ocr_rt_device_count(void);
/* How the library's host threads wait for their streams (process-wide; round 6): 1 = block on an event created with
 * hipEventBlockingSync (the thread sleeps until the interrupt; default), 0 = hipStreamSynchronize's spin (what rounds 1-5 did:
 * three spinning host threads per pipeline handle, 24 busy cores for the eight ranks of a node).  OCR_WAIT_MODE=spin|block in
 * the environment sets the initial mode.  The reference has no counterpart: its workers wait inside Paddle's predictor. */
int ocr_rt_set_wait_mode(int mode);
int ocr_rt_get_wait_mode(void);

/* An image view: CV_8UC3 BGR rows, possibly a non-contiguous ROI (row_stride in bytes) —
 * the `const cv::Mat&` of the reference signatures. */
typedef struct ocr_img {
  const uint8_t* data;
  int rows, cols;
  size_t row_stride;
} ocr_img;

/* ---------------------------------------------------------------- detector */
/* Field-for-field the constructor arguments of DBDetector (ocr_det.h:60-75) that still mean
 * something without Paddle; defaults of ocr_det_cfg_default() are the literals OCRWorker passes
 * (ocr_worker.cpp:21-35: "max", 512, 0.2, 0.4, 1.8, "fast", no dilation). */
typedef struct ocr_det_cfg {
  const char* model_dir; /* directory holding inference.pdmodel + inference.pdiparams */
  int device_id;
  const char* limit_type; /* "max" | "min" */
  int limit_side_len;
  double det_db_thresh;
  double det_db_box_thresh;
  double det_db_unclip_ratio;
  const char* det_db_score_mode; /* "fast" | "slow" */
  int use_dilation;
  /* "fp32": the bit-exact arithmetic contract (default).  "fp16": the reference's TensorRT precision switch
   * (ocr_det.cpp:50-56) - activation tensors stored as f16, matrix-core products as f16 instructions with f32 accumulation,
   * every other chain and reduction in f32: results within a stated tolerance of fp32, not identical.
   * "int8" is rejected. */
  const char* precision;
  int max_batch;         /* images per ocr_det_run_batch call the handle is sized for (>=1) */
  /* Which OpenCV the reference binary was built against, where two 4.x releases differ on this path (DESIGN.md
   * section 5).  Today one rule depends on it: cv::fillPoly's scan fill behind BoxScoreFast / PolygonScoreAcc
   * (postprocess_op.cpp:205-251) - OCR_CV_45: the rule of OpenCV 4.0 - 4.5.1, spans [ceil(xa), floor(xb)] of unshifted
   * edges; OCR_CV_410: the rule of 4.5.2 and later (edges moved by half a pixel, spans [floor, floor]).  0 = default:
   * the environment variable OCR_CV_COMPAT ("45" | "410") if set, else OCR_CV_410 - the reference's README builds with
   * a 2025 MSVC toolchain against vcpkg's current opencv port (README.md:105-118). */
  int cv_compat;
} ocr_det_cfg;
#define OCR_CV_DEFAULT 0
#define OCR_CV_45 45
#define OCR_CV_410 410
void ocr_det_cfg_default(ocr_det_cfg* cfg);

typedef struct ocr_det ocr_det;
int ocr_det_create(const ocr_det_cfg* cfg, ocr_det** out);
void ocr_det_destroy(ocr_det* h);
/* DBDetector::Run for one image.  boxes: cap x 8 int32 (4 points x,y clockwise from top-left, source
 * image coordinates), *n = boxes found; times[3] = pre / infer / post in ms (ocr_det.cpp:168-175). */
int ocr_det_run(ocr_det* h, const ocr_img* img, int32_t* boxes, int cap, int* n, double times[3]);
/* Same for `count` images of identical size in one device pass (batch on the GEMM row axis).
 * boxes: count x cap x 8; n: count entries. */
int ocr_det_run_batch(ocr_det* h, const ocr_img* imgs, int count, int32_t* boxes, int cap, int* n, double times[3]);
/* Parity taps: sizes of the network input of the last run, its probability map (rows*cols f32)
 * and bitmap. */
int ocr_det_last_shape(ocr_det* h, int* count, int* rows, int* cols);
int ocr_det_prob_map(ocr_det* h, int index, float* out, size_t cap_floats);
int ocr_det_bitmap(ocr_det* h, int index, uint8_t* out, size_t cap_bytes);
int ocr_det_resized(ocr_det* h, int index, uint8_t* out, size_t cap_bytes); /* u8 BGR after ResizeImgType0 */
/* Post-processing alone on a caller-supplied probability map (rows x cols f32, values in [0,1]):
 * threshold (+dilate) -> contours -> boxes -> FilterTagDetRes against a src_rows x src_cols image. */
int ocr_det_post(ocr_det* h, const float* prob, int rows, int cols, int src_rows, int src_cols, int32_t* boxes, int cap,
                 int* n);

/* ---------------------------------------------------------------- classifier */
typedef struct ocr_cls_cfg {
  const char* model_dir;
  int device_id;
  double cls_thresh; /* stored, never consulted — as in the reference (ocr_cls.cpp never reads it) */
  int cls_batch_num;
  const char* precision;
} ocr_cls_cfg;
void ocr_cls_cfg_default(ocr_cls_cfg* cfg);
typedef struct ocr_cls ocr_cls;
int ocr_cls_create(const ocr_cls_cfg* cfg, ocr_cls** out);
void ocr_cls_destroy(ocr_cls* h);
/* Classifier::Run: labels/scores are caller-sized to n (ocr_worker.cpp:271-272). */
int ocr_cls_run(ocr_cls* h, const ocr_img* imgs, int n, int* labels, float* scores, double times[3]);
/* tap: softmax [n][2] of the last run */
int ocr_cls_probs(ocr_cls* h, float* out, size_t cap_floats);

/* ---------------------------------------------------------------- recognizer */
typedef struct ocr_rec_cfg {
  const char* model_dir;
  int device_id;
  const char* label_path; /* ppocr_keys_v1.txt; "#"/" " are added like ocr_rec.h:82-84 */
  int rec_batch_num;
  int rec_img_h, rec_img_w;
  const char* precision;
  /* how lines with EQUAL w/h ratio are ordered before the batches of rec_batch_num are cut (Utility::argsort is
   * std::sort, utility.cpp:192-203, whose order of ties is the host library's): OCR_SORT_STD = this build's
   * std::sort (libstdc++ introsort, what the oracle runs); OCR_SORT_STABLE = ties keep their input order, which is
   * what MSVC's std::sort (the reference's toolchain) does for up to 32 crops (insertion sort below _ISORT_MAX).  Beyond 32
   * crops of one image MSVC's quicksort order of ties is NOT restated: OCR_SORT_STABLE keeps input order there too (a
   * documented choice, not MSVC's order); OCR_SORT_MSVC_STRICT is OCR_SORT_STABLE that REFUSES such an image - more than 32
   * crops of which two have equal ratios - with OCR_ERR_ARG and a message naming the image, instead of answering in an
   * order the reference's build may not produce. */
  int sort_mode;
} ocr_rec_cfg;
enum { OCR_SORT_STD = 0, OCR_SORT_STABLE = 1, OCR_SORT_MSVC_STRICT = 2 };
void ocr_rec_cfg_default(ocr_rec_cfg* cfg);
typedef struct ocr_rec ocr_rec;
int ocr_rec_create(const ocr_rec_cfg* cfg, ocr_rec** out);
void ocr_rec_destroy(ocr_rec* h);
/* CRNNRecognizer::Run.  For line i: ids[i*max_len .. +lens[i]) are the kept CTC class ids
 * (dictionary indices, blank and repeats removed), scores[i] the mean max-probability.  Lines the
 * reference leaves untouched (NaN score: no kept step) get lens[i] = 0, scores[i] = 0. */
int ocr_rec_run(ocr_rec* h, const ocr_img* imgs, int n, int32_t* ids, int max_len, int* lens, float* scores,
                double times[3]);
/* ocr_rec_run plus, per kept character (arrays parallel to ids, n x max_len): its CTC step, the length of its run of
 * equal arg maxes, and the max-probability of that step; per line geom[3] = {T, tensor_w, resize_w}; and, when topk > 0,
 * the topk best classes of that step's logits row (n x max_len x topk, rank-major per character). Any of steps/nsteps/
 * probs/geom may be NULL; topk == 0 ignores alt_*.  topk is 0..8 (else OCR_ERR_ARG).
 * ids / lens / scores are ocr_rec_run's, bit for bit, for every topk; probs[j] is the exact term of the score sum.
 * Ranking: by logit, descending; equal logits rank the lower class first (the head's own "first maximum"), so rank 0 is
 * the character's id; NaN ranks last.  A character's column span on the line's tensor is [step * tensor_w / T,
 * (step + nsteps) * tensor_w / T), of which [0, resize_w) holds the resized crop.
 * alt_probs: rank 0 is probs[j], the same bits.  Rank r > 0 is ocr_expf(x_r - x_0) * probs[j], an ESTIMATE of the softmax
 * probability that is NOT part of the bit-exact contract (the head's exp clamps its argument at -87; the relative error
 * is the head's own plus a few ulps).  Ranks a row does not have: id -1, prob 0.
 * topk > 0 keeps the recognizer's logits in device memory (the mobile head runs unfused, the server head without its CTC
 * partials): the call costs more than ocr_rec_run, and switching between topk > 0 and topk == 0 re-binds the network. */
int ocr_rec_run_chars(ocr_rec* h, const ocr_img* imgs, int n, int32_t* ids, int max_len, int* lens, float* scores,
                      int32_t* steps, int32_t* nsteps, float* probs, int32_t* geom,
                      int topk, int32_t* alt_ids, float* alt_probs, double times[3]);
/* tap: the logits row the top-k kernel read for step `step` of line `index` of the last ocr_rec_run_chars(topk > 0) */
int ocr_rec_logits_row(ocr_rec* h, int index, int step, float* out, size_t cap_floats);
/* self-test: the top-k kernel alone on caller rows (n rows of C f32 at `pitch` floats), p0[n] the rank-0 probability */
int ocr_selftest_topk(const float* rows, int n, int C, int pitch, const float* p0, int k, int32_t* out_ids, float* out_probs);
/* UTF-8 label of a class id (valid until the handle is destroyed); NULL when out of range. */
const char* ocr_rec_label(ocr_rec* h, int id);
int ocr_rec_num_classes(ocr_rec* h);
/* tap: per-step arg max / max prob of line `index` of the last run (T entries), and T */
int ocr_rec_steps(ocr_rec* h, int index, int32_t* amax, float* pmax, int cap, int* T);
/* self-test: at most n lines per recognizer launch from the next run on (a mobile recognizer: a launch's pixel budget is that of
 * n lines of rec_img_h x max(rec_img_w, 320)).  A call is cut into as many launches as that takes; its results do not depend on
 * the cut.  n < 1 is OCR_ERR_ARG and leaves the handle as it was.  No environment switch sets it; the default stays. */
int ocr_rec_set_launch_lines(ocr_rec* h, int n);
/* self-test, server recognizer only (OCR_ERR_ARG otherwise): HIP events around the network's launches (enable resets the rows), and one row per launch name,
 * "name ms count flops bytes" - the format of ocr_net_timing_report.  A launch's name carries the shape it was bound to, and
 * its count is the number of times it ran: what tells how many launches a call was cut into. */
int ocr_rec_timing(ocr_rec* h, int enable);
int ocr_rec_timing_report(ocr_rec* h, char* buf, size_t cap);


/* ---------------------------------------------------------------- pipeline */
/* OCRWorker::processRequest (/root/reference/src/ocr_worker.cpp:213-311) for a batch of images in one
 * device pass: det -> crops (crop_mode) -> [cls -> in-place 180 degree rotation] -> rec -> CTC.
 * The three stage handles live on one device; images are uploaded once and the crops are taken
 * from the device copy (the reference's ROI views of the request's cv::Mat clone). */
typedef struct ocr_pipe_cfg {
  ocr_det_cfg det;
  ocr_cls_cfg cls;
  ocr_rec_cfg rec;
  int enable_cls; /* OCRWorker(..., enable_cls = false) */
  int crop_mode;  /* OCR_CROP_BOUNDING_RECT: ROI views, what the worker does (ocr_worker.cpp:244-259);
                   * OCR_CROP_ROTATE: Utility::GetRotateCropImage per box (utility.cpp:137-190) */
  int phases;     /* chains a batch is run on, 1..4 (0 = the default, 2): the batch is cut into that many parts that run side by
                   * side, each with its own stage objects, streams and host thread (the latency-bound phases of one run
                   * under the dense kernels of another; results are per image and do not change); 1 = one chain, one
                   * kernel at a time owns the device.  OCR_PIPE_PHASES in the environment overrides. */
} ocr_pipe_cfg;
enum { OCR_CROP_BOUNDING_RECT = 0, OCR_CROP_ROTATE = 1 };
void ocr_pipe_cfg_default(ocr_pipe_cfg* cfg);
/* WordResult (ocr_worker.h:34-38): text as class ids ids[ids_off .. ids_off+ids_len) */
typedef struct ocr_word {
  int32_t box[8];
  int32_t ids_off, ids_len;
  float confidence;
} ocr_word;
/* One kept character of a word (ocr_pipe_run_chars): its CTC step and run length, the max-probability of that step, and
 * its quad in SOURCE-IMAGE coordinates (4 points x,y: top-left, top-right, bottom-right, bottom-left in reading orientation). */
typedef struct ocr_char {
  int32_t step, nsteps;
  float prob;
  int32_t quad[8];
} ocr_char;
typedef struct ocr_pipe ocr_pipe;
int ocr_pipe_create(const ocr_pipe_cfg* cfg, ocr_pipe** out);
void ocr_pipe_destroy(ocr_pipe* h);
/* imgs: `count` images (any mix of sizes).  Images of equal size share one det pass; the text lines of ALL images
 * then go through one cls pass and one rec pass (each image's lines are still sorted and cut into batches of
 * rec_batch_num on their own, ocr_rec.cpp:34-57: results do not depend on what else is in the call).
 * words: cap_words entries, image i owns words[word_off[i] .. word_off[i]+nwords[i]); ids: cap_ids class ids.
 * times[3] = det / cls / rec wall ms.  = ocr_pipe_stage(slot 0) + ocr_pipe_run_staged(slot 0). */
int ocr_pipe_run(ocr_pipe* h, const ocr_img* imgs, int count, ocr_word* words, int cap_words, int* word_off, int* nwords,
                 int32_t* ids, int cap_ids, double times[3]);
/* The same with inputs already resident in HBM: `count` packed BGR images of rows x cols (one every
 * rows*cols*3 bytes, device pointer), and optionally `dev_prob` = count probability maps of the
 * detector's input resolution that replace the network's map for thresholding/scoring (benchmark
 * protocol for synthetic weights; the network still runs and is timed). */
int ocr_pipe_run_device(ocr_pipe* h, const void* dev_bgr, int rows, int cols, int count, const float* dev_prob, ocr_word* words,
                        int cap_words, int* word_off, int* nwords, int32_t* ids, int cap_ids, double times[3]);
/* Double-buffered input: ocr_pipe_stage copies the host images into pinned memory (a few
 * host threads) and starts their upload on a copy stream, then returns; ocr_pipe_run_staged waits for that upload on
 * the device and runs the batch.  Two slots (0, 1): one host thread stages batch k+1 into the other slot while
 * another is inside ocr_pipe_run_staged for batch k; a slot may be run any number of times (its images then are
 * "already resident in HBM").
 * ocr_pipe_slot_probs (benchmark protocol): per staged image a pointer (host or device memory) to a probability map
 * of the detector's input resolution (ocr_pipe_det_shape) that replaces the network's map, as dev_prob of
 * ocr_pipe_run_device; the maps stay attached while the slot is re-staged with the same sizes in the same order. */
int ocr_pipe_stage(ocr_pipe* h, int slot, const ocr_img* imgs, int count);
int ocr_pipe_slot_probs(ocr_pipe* h, int slot, const float* const* probs, int count);
int ocr_pipe_run_staged(ocr_pipe* h, int slot, ocr_word* words, int cap_words, int* word_off, int* nwords, int32_t* ids,
                        int cap_ids, double times[3]);
/* Two batches in flight on one handle (round 5).  The reference's throughput shape is a pool of workers on one GPU
 * (/root/reference/src/gpu_worker_pool.cpp:12-16 pins every worker to GPU 0, ocr_worker.cpp:213-311 runs one request at a
 * time per worker): consecutive requests overlap, the halves of one request do not.  The `_on` forms run the WHOLE batch on
 * ONE of the handle's chains (0 <= chain < ocr_pipe_cfg.phases, default 2; own stage objects, streams, arenas and clone
 * buffer per chain) instead of cutting it over all of them.  Calls that name different chains - and, for the staged form,
 * different slots - may run concurrently from different host threads: chain 0 works on batch k while chain 1 works on
 * batch k+1, each call returning its own batch's results.  Results are those of the plain calls (per image, independent
 * of the batch composition).  Two calls on the SAME chain (or slot) at once are the caller's error. */
int ocr_pipe_run_device_on(ocr_pipe* h, int chain, const void* dev_bgr, int rows, int cols, int count, const float* dev_prob,
                           ocr_word* words, int cap_words, int* word_off, int* nwords, int32_t* ids, int cap_ids, double times[3]);
int ocr_pipe_run_staged_on(ocr_pipe* h, int chain, int slot, ocr_word* words, int cap_words, int* word_off, int* nwords, int32_t* ids,
                           int cap_ids, double times[3]);
/* ocr_pipe_run plus one ocr_char per class id (chars parallel to ids, cap_ids entries); words / ids are ocr_pipe_run's bit
 * for bit.  The quad is host arithmetic in double on the line's own geometry: with s = tensor_w / T the character spans
 * tensor columns [step * s, (step + nsteps) * s), clipped to [0, resize_w] and scaled by crop_w / resize_w into crop x; it
 * takes the full crop height; a crop the classifier turned by 180 degrees is mirrored in x and y first; then back into
 * the image - OCR_CROP_BOUNDING_RECT: plus the crop rectangle's origin; OCR_CROP_ROTATE: the 90-degree turn undone, then
 * the crop's own inverse homography (csrc/crop.h).  Corners are rounded half up and clamped to [0, cols-1] x [0, rows-1]. */
int ocr_pipe_run_chars(ocr_pipe* h, const ocr_img* imgs, int count, ocr_word* words, int cap_words, int* word_off,
                       int* nwords, int32_t* ids, int cap_ids, ocr_char* chars /* parallel to ids */, double times[3]);
/* JPEG inputs with the pixel half of the decoder on the device: the caller runs the
 * bit-serial entropy decoding (host/jpeg_decode.h, Decoder::decode_coefficients) and hands over quantised DCT
 * coefficients; dequantisation, IDCT, chroma upsampling and colour conversion run on the copy stream straight into
 * the slot - otherwise exactly ocr_pipe_stage.  Results equal decoding on the host first, bit for bit. */
typedef struct ocr_jpeg_comp {
  const int16_t* coef; /* host: bw*bh blocks x 64 quantised coefficients, blocks row-major, natural order inside */
  uint16_t quant[64];  /* quantisation table, natural order */
  int bw, bh;          /* blocks per row / column (padded to whole MCUs) */
  int dw, dh;          /* component size in samples: ceil(cols*h/hmax), ceil(rows*v/vmax) */
} ocr_jpeg_comp;
typedef struct ocr_jpeg_img {
  int rows, cols, ncomp; /* STORED size (the SOF's); ncomp 1 (grey) or 3 (YCbCr) */
  int hmax, vmax;        /* luma sampling factors, chroma 1x1: 1x1 (4:4:4), 2x1 (4:2:2), 2x2 (4:2:0) */
  /* EXIF Orientation (tag 0x0112 in IFD0 of the file's first Exif APP1 segment), applied to the decoded pixels as
   * cv::imdecode does: 0 or 1 = as stored, 2..8 = the table in host/jpeg_decode.h; anything else is refused
   * (OCR_ERR_ARG).  rows / cols stay the stored size: for 5..8 the image that ocr_jpeg_decode writes and the slot
   * image of ocr_pipe_stage_jpeg are cols x rows.  Producers zero-initialise the struct.  The field sits in what
   * was alignment padding in front of comp[] (the pointer in ocr_jpeg_comp aligns it to 8): size and every other
   * offset are unchanged, and a caller built against the older header that zeroed the struct keeps its behaviour. */
  int orientation;
  ocr_jpeg_comp comp[3];
} ocr_jpeg_img;
/* (kept for callers built against it: every image becomes the ocr_jpeg_frame that says the same and goes through
 * ocr_pipe_stage_frames' code; new callers use that entry point) */
int ocr_pipe_stage_jpeg(ocr_pipe* h, int slot, const ocr_jpeg_img* imgs, int count);
/* the same device decode of one image with the pixels copied back to the host (tests, tools) */
int ocr_jpeg_decode(const ocr_jpeg_img* img, int device_id, uint8_t* bgr, size_t cap_bytes);
/* measurement aid (decode_tool --time): the two kernels of that decode, each launched `iters` times between HIP events
 * after one untimed decode; ms[0] = mean of the IDCT launch, ms[1] = mean of the pixel stage (upsampling, colour,
 * orientation). */
int ocr_jpeg_time(const ocr_jpeg_img* img, int device_id, int iters, double ms[2]);
/* The general descriptor: what ocr_jpeg_img (frozen: three components, chroma 1x1) cannot hold.  1, 3 or 4 components,
 * each with its own sampling factors h, v in 1..4 (luma included) where every hmax / h and vmax / v is integral, and the
 * colour space of the file by libjpeg's rule (host/jpeg_decode.h).  Upsampling per component as libjpeg-turbo's jdsample.c
 * chooses it (copy, fancy h2v1 / h2v2 / h1v2, box replication), YCCK -> CMYK as jdcolor.c, CMYK -> BGR as OpenCV.  An
 * image that ocr_jpeg_img can hold runs the same kernels through either descriptor, with the same result.  The three
 * entry points are the counterparts of the three above; a descriptor that breaks a rule stated here is refused
 * (OCR_ERR_ARG, ocr_last_error says which). */
typedef enum ocr_jpeg_color {
  OCR_JPEG_GREY = 0,  /* ncomp 1 */
  OCR_JPEG_YCBCR = 1, /* ncomp 3 */
  OCR_JPEG_RGB = 2,   /* ncomp 3: stored as R, G, B (Adobe transform 0, or component ids 'R','G','B') */
  OCR_JPEG_CMYK = 3,  /* ncomp 4: libjpeg's raw samples */
  OCR_JPEG_YCCK = 4   /* ncomp 4: Adobe transform 2 */
} ocr_jpeg_color;
typedef struct ocr_jpeg_fcomp {
  const int16_t* coef; /* as ocr_jpeg_comp */
  uint16_t quant[64];
  int bw, bh;          /* blocks per row / column; bw * 8 >= dw, bh * 8 >= dh */
  int dw, dh;          /* component size in samples: ceil(cols*h/hmax), ceil(rows*v/vmax) */
  int h, v;            /* sampling factors 1..4; 1, 1 for a single component */
} ocr_jpeg_fcomp;
typedef struct ocr_jpeg_frame {
  int rows, cols, ncomp; /* STORED size; ncomp 1, 3 or 4 */
  int orientation;       /* as ocr_jpeg_img.orientation */
  int color;             /* ocr_jpeg_color, consistent with ncomp */
  int reserved;          /* 0 */
  ocr_jpeg_fcomp comp[4];
} ocr_jpeg_frame;
/* ocr_pipe_stage_frames (below) for JPEG frames only, handed over as an array */
int ocr_pipe_stage_jpeg_frames(ocr_pipe* h, int slot, const ocr_jpeg_frame* frames, int count);
/* the staged image that was imgs[index] / frames[index] of the slot's last stage call, copied back to the host as
 * packed BGR (tests, tools: what a stage call put into the slot, whichever kernels wrote it); rows / cols: its size */
int ocr_pipe_slot_image(ocr_pipe* h, int slot, int index, uint8_t* bgr, size_t cap_bytes, int* rows, int* cols);
int ocr_jpeg_decode_frame(const ocr_jpeg_frame* frame, int device_id, uint8_t* bgr, size_t cap_bytes);
int ocr_jpeg_time_frame(const ocr_jpeg_frame* frame, int device_id, int iters, double ms[2]);
/* PNG inputs with the pixel half of the decoder on the device, the counterpart of the JPEG descriptors: the caller
 * parses the container and inflates the IDAT stream (host/png_decode.h, png::parse); unfiltering, conversion and Adam7
 * placement run on the copy stream straight into the slot.  The pixels are cv::imdecode(IMREAD_COLOR)'s: a 16-bit
 * sample keeps its high byte, alpha is dropped (nothing is composited), depths 1 / 2 / 4 are expanded by bit
 * replication, palette indices go through `palette`, grey fills three channels, no gamma.  Every field is checked on the
 * host before anything is launched (OCR_ERR_ARG, ocr_last_error says which rule). */
typedef struct ocr_png_segment {
  int32_t pass;      /* 0 when not interlaced, else the Adam7 pass 0..6 */
  int32_t first_row; /* row of that pass */
  int32_t rows;      /* >= 1 */
} ocr_png_segment;
typedef struct ocr_png_frame {
  int width, height;     /* IHDR; width * height <= 64 Mpixel */
  int bit_depth;         /* 1, 2, 4, 8, 16 as the colour type allows */
  int color_type;        /* 0, 2, 3, 4, 6 */
  int interlace;         /* 0, or 1 = Adam7 */
  int reserved;          /* 0 */
  uint8_t palette[768];  /* R, G, B x 256; zero beyond PLTE */
  const uint8_t* data;   /* host: the inflated stream - per non-empty pass, per row, a filter byte (0..4) and the filtered bytes */
  size_t data_len;       /* exactly what IHDR implies: sum over passes of rows * (1 + rowbytes) */
  /* Maximal runs of rows that never look at a row outside the run, in stream order: a run starts at the first row of a
   * (non-empty) pass or at a row whose filter is None (0) or Sub (1); together they cover every row once. */
  const ocr_png_segment* segments;
  int nsegments;         /* at most 65536, and no pass with more than 16384 rows: beyond that the decode belongs on the host */
} ocr_png_frame;
int ocr_png_decode(const ocr_png_frame* frame, int device_id, uint8_t* bgr, size_t cap_bytes);
/* measurement aid (decode_tool --time): after one untimed decode, `iters` repetitions between HIP events of ms[0] = the
 * upload of the inflated stream from pinned memory, ms[1] = the pixel-stage kernel (means per repetition).
 * ocr_png_time_batch: the same for `count` frames as ONE batch (one upload, one launch per bpp kind), per batch. */
int ocr_png_time(const ocr_png_frame* frame, int device_id, int iters, double ms[2]);
int ocr_png_time_batch(const ocr_png_frame* const* frames, int count, int device_id, int iters, double ms[2]);
/* ocr_pipe_stage_frames (below) without raw frames: image i is jpegs[i] or pngs[i], exactly one of the two non-null (either
 * array may be NULL when no image of the batch uses it). */
int ocr_pipe_stage_coded(ocr_pipe* h, int slot, const ocr_jpeg_frame* const* jpegs, const ocr_png_frame* const* pngs, int count);
/* BMP and PNM inputs with the pixel half of the decoder on the device: the caller parses the container and does what is
 * serial (run-length expansion, ASCII numbers: host/raw_decode.h, raw::parse); bit, nibble and palette expansion, 5-5-5 /
 * 5-6-5, the high bytes of 16-bit samples, row order and channel order run on the copy stream straight into the slot.
 * The pixels are cv::imdecode(IMREAD_COLOR)'s.  Every field is checked on the host before anything is launched
 * (OCR_ERR_ARG, ocr_last_error says which rule). */
typedef enum ocr_raw_kind {
  OCR_RAW_INDEX1, OCR_RAW_INDEX4, OCR_RAW_INDEX8,   /* through palette; most significant bit / high nibble first */
  OCR_RAW_BGR555, OCR_RAW_BGR565,                   /* 16-bit little-endian, expanded by shifting: low bits 0 */
  OCR_RAW_BGR24,  OCR_RAW_BGRX32, OCR_RAW_RGB24,
  OCR_RAW_GREY8,  OCR_RAW_GREY16BE, OCR_RAW_RGB48BE, /* 16-bit big-endian: the high byte is kept */
  OCR_RAW_BIT1_INV                                  /* PBM: 1 = black */
} ocr_raw_kind;
typedef struct ocr_raw_frame {
  int width, height;       /* width * height <= 64 Mpixel */
  int kind;                /* ocr_raw_kind */
  int bottom_up;           /* 1: stored row r is image row height - 1 - r */
  size_t row_stride;       /* bytes between stored rows, >= the row's own bytes, <= 2 GiB */
  uint8_t palette[1024];   /* B,G,R,x times 256; zero beyond the file's */
  const uint8_t* data;     /* host */
  size_t data_len;         /* >= (height-1)*row_stride + row bytes */
} ocr_raw_frame;
int ocr_raw_decode(const ocr_raw_frame* frame, int device_id, uint8_t* bgr, size_t cap_bytes);
/* measurement aid (decode_tool --time), as ocr_png_time: ms[0] = the upload of the stored rows from pinned memory,
 * ms[1] = the pixel-stage kernel; ocr_raw_time_batch: `count` frames as ONE batch (one upload, one launch per kind). */
int ocr_raw_time(const ocr_raw_frame* frame, int device_id, int iters, double ms[2]);
int ocr_raw_time_batch(const ocr_raw_frame* const* frames, int count, int device_id, int iters, double ms[2]);
/* THE staging entry point for coded images - what new callers use: a batch of JPEG, PNG and raw frames in any mix.  Image i
 * is jpegs[i], pngs[i] or raws[i], exactly one of the three non-null (an array may be NULL when no image of the batch uses it).
 * ocr_pipe_stage_jpeg (every image an ocr_jpeg_img), ocr_pipe_stage_jpeg_frames (an array of JPEG frames) and
 * ocr_pipe_stage_coded (no raws) are kept as equivalents: they validate their own argument list and stage through the same
 * code, with the same bytes in the slot. */
int ocr_pipe_stage_frames(ocr_pipe* h, int slot, const ocr_jpeg_frame* const* jpegs, const ocr_png_frame* const* pngs,
                          const ocr_raw_frame* const* raws, int count);
/* TIFF inputs with the pixel half of the decoder on the device: the caller parses the container and does what is serial
 * (the IFD, PackBits / LZW / Deflate expansion, FillOrder: host/tiff_decode.h, tiff::parse); the horizontal-differencing
 * predictor (a scan along each chunk row), tile placement with clipped edge tiles, planar to chunky, 1- / 2- / 4-bit expansion,
 * palette, MinIsWhite, 16 -> 8 bits, CMYK and alpha run on the copy stream straight into the slot.  The pixels are
 * cv::imdecode(IMREAD_COLOR)'s as libtiff's RGBA interface makes them.  Every field is checked on the host before anything
 * is launched (OCR_ERR_ARG, ocr_last_error says which rule). */
typedef struct ocr_tiff_frame {
  int width, height;       /* width * height <= 64 Mpixel */
  int photometric;         /* 0 MinIsWhite, 1 MinIsBlack, 2 RGB, 3 palette, 5 CMYK */
  int bits_per_sample;     /* 1, 2, 4 (grey, palette: one sample, chunky, no predictor), 8, 16 (not palette, not CMYK) */
  int samples_per_pixel;   /* as stored, extra samples included: 1 .. 16, at least the photometric's 1 / 3 / 4 */
  int planar;              /* 1 chunky; 2 one plane of chunks per sample (RGB, or grey with extra samples) */
  int predictor;           /* 1; 2: samples are differences from the pixel before in the chunk's row (8 and 16 bits) */
  int big_endian;          /* of 16-bit samples: the predictor's sum runs on the words in this order */
  int premultiply;         /* 1: the sample behind the colour is unassociated alpha, c = (c * a + 127) / 255 (RGB; grey in planes) */
  int tile_width, tile_height; /* a chunk; a strip is a chunk as wide as the image and min(RowsPerStrip, height) high */
  uint8_t palette[1024];   /* B,G,R,x times 256, reduced to 8 bits */
  const uint8_t* data;     /* host: the expanded chunks, each at its nominal size tile_height * row bytes, plane by plane, row of
                            * chunks by row of chunks */
  size_t data_len;         /* >= planes * chunks * tile_height * row bytes, which is <= 1 GiB */
} ocr_tiff_frame;
int ocr_tiff_decode(const ocr_tiff_frame* frame, int device_id, uint8_t* bgr, size_t cap_bytes);
/* measurement aid (decode_tool --time), as ocr_raw_time: ms[0] = the upload of the chunks from pinned memory, ms[1] = the
 * pixel-stage kernel; ocr_tiff_time_batch: `count` frames as ONE batch (one upload, one launch per sample width). */
int ocr_tiff_time(const ocr_tiff_frame* frame, int device_id, int iters, double ms[2]);
int ocr_tiff_time_batch(const ocr_tiff_frame* const* frames, int count, int device_id, int iters, double ms[2]);
/* TIFF inputs with the expansion of the chunks on the device as well (Compression 1, 5 = LZW, 32773 = PackBits): the caller
 * stops before the expansion (host/tiff_decode.h, tiff::parse_coded) and hands over coded bytes - the frame without `data`, one
 * record per chunk in the order `data` would have them, and one pool of the chunks' bytes, MSB first (FillOrder 2 undone).  A
 * chunk is expanded by one wavefront (csrc/kernels_tiff_lzw.hip) into device scratch, to the bytes of tiff::expand.  Every
 * field and every stream is checked on the host before anything is launched (tiff::coded_fault, which scans each chunk's codes
 * for the bytes its rows need: OCR_ERR_ARG, ocr_last_error says which rule); a frame of more than 2^20 chunks or 512 MiB of
 * chunks at their nominal size is refused here - tiff::expand and ocr_tiff_decode take it. */
typedef struct ocr_tiff_chunk {
  uint64_t byte_off;  /* into bytes */
  uint32_t byte_len;
  uint32_t rows;      /* the rows the chunk really holds, 1 .. tile_height (the last strip may have fewer) */
} ocr_tiff_chunk;
typedef struct ocr_tiff_coded {
  ocr_tiff_frame frame;          /* data is NULL (data_len is not read) */
  int compression;               /* 1, 5 or 32773; 8 or 32946 for the Deflate entry points alone */
  const ocr_tiff_chunk* chunks;  /* host: plane by plane, row of chunks by row of chunks */
  size_t chunks_len;
  const uint8_t* bytes;          /* host */
  size_t bytes_len;
} ocr_tiff_coded;
/* the expansion alone: out[0 .. chunks * tile_height * row bytes) as tiff::parse fills Frame::data, zero rows behind a short
 * last strip included; cap in bytes */
int ocr_tiff_expand(const ocr_tiff_coded* coded, int device_id, uint8_t* out, size_t cap);
/* the expansion, then the launches of ocr_tiff_decode, on one stream with no host round trip in between */
int ocr_tiff_decode_coded(const ocr_tiff_coded* coded, int device_id, uint8_t* bgr, size_t cap_bytes);
/* measurement aid (decode_tool --time): ms[0] = the upload of the pool, records and descriptors from pinned memory, ms[1] = the
 * expansion, ms[2] = the pixel stage's kernels; ocr_tiff_time_coded_batch: `count` frames as ONE batch. */
int ocr_tiff_time_coded(const ocr_tiff_coded* coded, int device_id, int iters, double ms[3]);
int ocr_tiff_time_coded_batch(const ocr_tiff_coded* const* coded, int count, int device_id, int iters, double ms[3]);
/* Deflate TIFFs (Compression 8 and 32946) on the same structure: an ocr_tiff_coded with that compression (host/tiff_decode.h,
 * tiff::parse_deflate: the container alone, one zlib stream per chunk, FillOrder 2 undone), through entry points of their own.
 * Fields and chunk records are checked on the host before anything is launched (OCR_ERR_ARG, nothing launched, the output
 * untouched); NO stream is looked at there.  One wavefront inflates one chunk (csrc/kernels_inflate.hip) and reports the bytes
 * its stream gave; a chunk is good where that is what its rows need - zlib's verdict on the host (tiff::detail::inflate):
 * neither a wrong Adler-32 nor a missing trailer behind those bytes refuses it.  The counts come back to the host (4 bytes a
 * chunk, the one round trip of this route); where a chunk fell short the call returns OCR_ERR_ARG "deflate: a chunk's stream does
 * not hold the bytes its rows need (frame F, chunk C)", no pixel kernel runs, the output's contents are unspecified and nothing
 * beyond its cap is written.  The caller's fallback is the host: tiff::inflate_all.
 * ocr_tiff_inflate: the expansion alone, out as ocr_tiff_expand's; produced (chunks_len words, may be NULL): the bytes each
 * chunk's stream gave, cut at what its rows need - it returns OCR_OK whatever the streams are, the verdict is in `produced`. */
int ocr_tiff_inflate(const ocr_tiff_coded* coded, int device_id, uint8_t* out, size_t cap, uint32_t* produced);
int ocr_tiff_decode_deflate(const ocr_tiff_coded* coded, int device_id, uint8_t* bgr, size_t cap_bytes);
/* measurement aid (decode_tool --time): ms[0] = the upload, ms[1] = the inflate launch with the read-back of its counts,
 * ms[2] = the pixel stage's kernels; ocr_tiff_time_deflate_batch: `count` frames as ONE batch. */
int ocr_tiff_time_deflate(const ocr_tiff_coded* coded, int device_id, int iters, double ms[3]);
int ocr_tiff_time_deflate_batch(const ocr_tiff_coded* const* coded, int count, int device_id, int iters, double ms[3]);
/* CCITT fax TIFFs (Compression 2 and 32771: Modified Huffman RLE; 3: T.4 / Group 3; 4: T.6 / Group 4) through entry points
 * of their own: the caller stops before the expansion (host/tiff_decode.h, tiff::parse_fax) and hands over the frame - 1 bit,
 * 1 sample, photometric 0 or 1 - with one record per strip or tile, the coding and the T4 options.  One chunk is expanded by
 * one wavefront (csrc/kernels_tiff_fax.hip) into device scratch, to the bytes of tiff::unfax_all: rows of 1-bit pixels, white 0
 * and black 1, which the 1-bit grey pixel stage takes.  Every field and every stream is checked on the host before anything
 * is launched (tiff::fax_fault_of, which walks each chunk's codes with the decoder's own verdict: OCR_ERR_ARG, ocr_last_error
 * says which rule, nothing launched, the output untouched).  A chunk wider than 8192 pixels and a frame beyond the bounds of
 * ocr_tiff_coded are refused here - tiff::unfax_all and ocr_tiff_decode take them. */
typedef struct ocr_tiff_fax {
  ocr_tiff_coded coded;  /* compression 2, 3, 4 or 32771 */
  uint32_t t4_options;   /* T4Options of Compression 3 (bit 0: two-dimensional; bit 2: fill bits), else 0 */
} ocr_tiff_fax;
/* the expansion alone, out as ocr_tiff_expand's */
int ocr_tiff_unfax(const ocr_tiff_fax* fax, int device_id, uint8_t* out, size_t cap);
/* the expansion, then the launches of ocr_tiff_decode, on one stream with no host round trip in between */
int ocr_tiff_decode_fax(const ocr_tiff_fax* fax, int device_id, uint8_t* bgr, size_t cap_bytes);
/* measurement aid (decode_tool --time): ms[0] = the upload, ms[1] = the expansion, ms[2] = the pixel stage's kernels;
 * ocr_tiff_time_fax_batch: `count` frames as ONE batch. */
int ocr_tiff_time_fax(const ocr_tiff_fax* fax, int device_id, int iters, double ms[3]);
int ocr_tiff_time_fax_batch(const ocr_tiff_fax* const* fax, int count, int device_id, int iters, double ms[3]);
/* Lossless WebP inputs with the pixel half of the decoder on the device: the caller parses the container and does what is
 * serial (prefix codes, LZ77, the colour cache: host/webp_decode.h, webp::parse); the inverse transforms - spatial predictor,
 * cross-colour, add-green, palette with pixel bundling - run on the copy stream straight into the slot.  The pixels are
 * cv::imdecode(IMREAD_COLOR)'s as libwebp's WebPDecodeBGR makes them (alpha dropped).  The device stage takes every order of
 * transforms in which colour indexing, if present, is the FIRST of the file (every order libwebp's encoder writes); another
 * order is refused here and finished on the host (webp::pixels).  Every field is checked on the host before anything is
 * launched (OCR_ERR_ARG, ocr_last_error says which rule). */
typedef struct ocr_webp_transform {
  int kind;              /* 0 predictor, 1 cross-colour, 2 add-green, 3 colour indexing; each at most once */
  int bits;              /* predictor, cross-colour: blocks of 2^bits pixels square, 2 .. 9; add-green: 0; colour indexing: a coded
                          * pixel holds 2^bits indices - 3 / 2 / 1 / 0 for <= 2 / <= 4 / <= 16 / more colours */
  const uint32_t* data;  /* host: predictor - the sub-image, mode in bits 8 .. 11; cross-colour - the sub-image, green-to-red,
                          * green-to-blue, red-to-blue in bytes 0, 1, 2; colour indexing - the palette, A << 24 | R << 16 | G << 8 | B,
                          * delta coding undone; add-green: unused */
  size_t data_len;       /* dwords: >= ceil(w / 2^bits) * ceil(height / 2^bits) for a sub-image (w: the width the transform works
                          * on - the coded width behind colour indexing); 1 .. 256 for the palette */
} ocr_webp_transform;
typedef struct ocr_webp_frame {
  int width, height;     /* 1 .. 16384 each, width * height <= 64 Mpixel */
  const uint32_t* argb;  /* host: the entropy-decoded image, A << 24 | R << 16 | G << 8 | B, coded width x height; the coded width
                          * is ceil(width / 2^bits) of the colour indexing transform, the width without one */
  size_t argb_len;       /* dwords: >= coded width * height */
  int ntransforms;       /* 0 .. 4 */
  ocr_webp_transform transforms[4]; /* in file order: they are undone last to first */
} ocr_webp_frame;
int ocr_webp_decode(const ocr_webp_frame* frame, int device_id, uint8_t* bgr, size_t cap_bytes);
/* measurement aid (decode_tool --time), as ocr_tiff_time: ms[0] = the upload of the coded data from pinned memory, ms[1] = the
 * pixel-stage kernels; ocr_webp_time_batch: `count` frames as ONE batch (one upload, one launch per kernel kind). */
int ocr_webp_time(const ocr_webp_frame* frame, int device_id, int iters, double ms[2]);
int ocr_webp_time_batch(const ocr_webp_frame* const* frames, int count, int device_id, int iters, double ms[2]);
/* Lossy WebP inputs (VP8 key frames) with the pixel half of the decoder on the device: the caller parses the container and
 * does what is serial (boolean decoder, headers, modes, tokens: host/vp8_decode.h, vp8::parse); inverse WHT and DCT, intra
 * prediction, the loop filter, fancy upsampling and the BGR conversion run on the copy stream straight into the slot.  The
 * pixels are cv::imdecode(IMREAD_COLOR)'s as libwebp's WebPDecodeBGR makes them.  The device stage takes every frame the host
 * half produces: nothing is left to the host.  Every field is checked on the host before anything is launched (OCR_ERR_ARG,
 * ocr_last_error says which rule). */
typedef struct ocr_vp8_mb {
  uint8_t modes[16];     /* is_i4x4: the sub-block modes 0 .. 9 (DC TM VE HE RD VR LD VL HD HU) in raster order; else modes[0] is the
                          * 16x16 mode 0 .. 3 (DC TM V H) */
  uint8_t is_i4x4;       /* 0 or 1 */
  uint8_t uvmode;        /* 0 .. 3 */
  uint8_t level;         /* loop filter level 0 .. 63 of this macroblock (segment and deltas applied); 0: not filtered */
  uint8_t ilevel;        /* interior limit, 0 .. 63 */
  uint8_t hev;           /* high edge variance threshold, 0 .. 2 */
  uint8_t inner;         /* 1: the inner edges are filtered too */
  uint8_t segment, skip; /* as coded; not read */
  uint32_t nz_y;         /* 2 bits a luma block, block 0 in bits 31 .. 30: 3 the full inverse DCT, 2 its three-coefficient form, else
                          * the DC form when the DC is not zero */
  uint32_t nz_uv;        /* the same for U (block 0 in bits 7 .. 6) and V (15 .. 14); a plane with any 2 or 3 is transformed in full */
  uint32_t present;      /* bit b: block b is shipped (0 .. 15 luma, 16 .. 19 U, 20 .. 23 V, 24 Y2; Y2 only when !is_i4x4) */
  uint32_t coeff_off;    /* in blocks of 16: the shipped blocks follow one another from here, in the order of their bits */
} ocr_vp8_mb;
typedef struct ocr_vp8_frame {
  int width, height;     /* 1 .. 16383 each */
  int filter_type;       /* 0 none, 1 simple (luma only), 2 normal */
  const ocr_vp8_mb* mbs; /* host: ceil(width / 16) * ceil(height / 16) records in raster order */
  size_t mbs_len;        /* records: >= that product */
  const int16_t* coeffs; /* host: dequantised coefficients, 16 a block in raster (not zigzag) order, as libwebp's int16_t holds them */
  size_t coeffs_len;     /* int16 values */
} ocr_vp8_frame;
int ocr_vp8_decode(const ocr_vp8_frame* frame, int device_id, uint8_t* bgr, size_t cap_bytes);
/* measurement aid (decode_tool --time), as ocr_webp_time: ms[0] = the upload of the descriptor from pinned memory, ms[1] = the
 * three kernels; ocr_vp8_time_batch: `count` frames as ONE batch (one upload, one launch per kernel kind). */
int ocr_vp8_time(const ocr_vp8_frame* frame, int device_id, int iters, double ms[2]);
int ocr_vp8_time_batch(const ocr_vp8_frame* const* frames, int count, int device_id, int iters, double ms[2]);
/* JPEG 2000 inputs with the sample half of the decoder on the device: the caller parses boxes and markers and does what is
 * serial (tier-2 packet headers, tier-1 MQ decoding: host/j2k_decode.h, j2k::parse); dequantisation, the multi-level inverse
 * wavelet transform (5/3 in int32, 9/7 in float32 in OpenJPEG's operation order), the inverse component transform, level shift,
 * clamp and the BGR store run on the copy stream straight into the slot.  The pixels are those of j2k::pixels, byte for byte.
 * A band's rectangle and the parity of its origin follow from the tile-component's rectangle (j2k::band_rect, j2k::res_rect).
 * The device stage takes frames of up to 8 decomposition levels whose tile's components share one level count; j2k::parse
 * says so in Frame::device_ok, other frames are finished on the host.  Every field is checked on the host before anything is
 * launched (OCR_ERR_ARG, ocr_last_error says which rule). */
typedef struct ocr_j2k_tilecomp {
  int x0, y0, x1, y1;   /* the tile-component's rectangle on the reference grid: inside the image, the same for the components of a tile */
  int levels;           /* decomposition levels, 0 .. 32 (the device stage: 0 .. 8) */
  int comp;             /* the file's component index; not read */
  uint32_t step_off;    /* into steps: 1 + 3 * levels values - LL, then HL, LH, HH of resolution 1, 2, ... (read by the 9/7 only) */
  uint32_t reserved;
  uint64_t coeff_off;   /* into coeffs: (x1 - x0) * (y1 - y0) values in the band arrangement, row stride x1 - x0 */
} ocr_j2k_tilecomp;
typedef struct ocr_j2k_frame {
  int width, height;    /* of the image; width * height <= 64 Mi */
  int x0, y0;           /* the image's origin on the reference grid (XOsiz, YOsiz) */
  int ncomp;            /* carried components per tile: 1 or 3 */
  int prec;             /* 1 .. 16; above 8 the samples are reduced by >> (prec - 8) */
  int transform;        /* 0: 5/3 reversible, 1: 9/7 */
  int mct;              /* 1: inverse component transform (RCT / ICT) over the three carried components */
  int chan[3];          /* which carried component is R, G, B */
  const ocr_j2k_tilecomp* tcs; /* host: ncomp records a tile, tiles in raster order, covering the image exactly */
  size_t tcs_len;
  const float* steps;   /* host: quantiser step sizes */
  size_t steps_len;
  const int32_t* coeffs; /* host: tier-1's integers with their half bit (units of half a step) */
  size_t coeffs_len;
} ocr_j2k_frame;
int ocr_j2k_decode(const ocr_j2k_frame* frame, int device_id, uint8_t* bgr, size_t cap_bytes);
/* measurement aid (decode_tool --time), as ocr_vp8_time: ms[0] = the upload of the descriptor from pinned memory, ms[1] = the
 * kernels; ocr_j2k_time_batch: `count` frames as ONE batch (one upload, two launches per level and one to finish). */
int ocr_j2k_time(const ocr_j2k_frame* frame, int device_id, int iters, double ms[2]);
int ocr_j2k_time_batch(const ocr_j2k_frame* const* frames, int count, int device_id, int iters, double ms[2]);
/* JPEG 2000 inputs with tier-1 on the device as well: the caller stops at the seam between tier-2 and tier-1
 * (host/j2k_decode.h, j2k::parse_coded) and hands over compressed bytes, not coefficients - the frame without `coeffs`, every
 * coded block with where its samples go, and one pool of the blocks' bytes.  A block is decoded by one wavefront, its state in
 * LDS (csrc/kernels_j2k_t1.hip); the coefficients are those of j2k::tier1, integer for integer.  Code-block style 0 only, as
 * j2k::parse.  Every field is checked on the host before anything is launched (j2k::coded_fault: OCR_ERR_ARG, ocr_last_error
 * says which rule); two blocks that overlap race on values and never leave the plane. */
typedef struct ocr_j2k_cblk {
  uint32_t tc;        /* index into the frame's tcs */
  uint32_t at;        /* sample offset of the block's top-left corner within its tile-component's plane (row stride x1 - x0) */
  uint64_t byte_off;  /* into bytes */
  uint32_t byte_len;  /* the block's chunks one after another, in layer order; bytes beyond read as ff */
  uint16_t w, h;      /* 1 .. 1024 each, w * h <= 4096, the rectangle inside the tile-component */
  uint8_t orient;     /* 0 LL, 1 HL, 2 LH, 3 HH */
  uint8_t numbps;     /* magnitude bit planes, 1 .. 30 */
  uint8_t passes;     /* coding passes, 1 .. 3 * numbps - 2 */
  uint8_t reserved;
  uint32_t reserved2;
} ocr_j2k_cblk;
typedef struct ocr_j2k_coded {
  ocr_j2k_frame frame;        /* coeffs is NULL, coeffs_len is the size of the coefficient plane tier-1 fills */
  const ocr_j2k_cblk* cblks;  /* host */
  size_t cblks_len;
  const uint8_t* bytes;       /* host */
  size_t bytes_len;
} ocr_j2k_coded;
/* tier-1 alone: coeffs[0 .. frame.coeffs_len) as j2k::tier1 fills them (samples outside every block: 0); cap in values */
int ocr_j2k_tier1(const ocr_j2k_coded* coded, int device_id, int32_t* coeffs, size_t cap);
/* tier-1, then the launches of ocr_j2k_decode, on one stream with no host round trip in between */
int ocr_j2k_decode_coded(const ocr_j2k_coded* coded, int device_id, uint8_t* bgr, size_t cap_bytes);
/* measurement aid (decode_tool --time): ms[0] = the upload of blocks, bytes and descriptors from pinned memory, ms[1] = zeroing
 * the plane and tier-1, ms[2] = the pixel stage's kernels; ocr_j2k_time_coded_batch: `count` frames as ONE batch. */
int ocr_j2k_time_coded(const ocr_j2k_coded* coded, int device_id, int iters, double ms[3]);
int ocr_j2k_time_coded_batch(const ocr_j2k_coded* const* coded, int count, int device_id, int iters, double ms[3]);
/* A batch as a tagged list: image i is frames[i].frame, a descriptor of the type frames[i].kind names - JPEG, PNG, raw, TIFF,
 * WebP, VP8 and JPEG 2000 frames (coefficient form and coded form) and coded TIFF frames in any mix.  ocr_pipe_stage_frames and the three entry points it lists stay as equivalents for the kinds they know:
 * all five validate their own argument list and stage through the same code, with the same bytes in the slot. */
typedef enum ocr_frame_kind { OCR_FRAME_JPEG = 0, OCR_FRAME_PNG = 1, OCR_FRAME_RAW = 2, OCR_FRAME_TIFF = 3, OCR_FRAME_WEBP = 4, OCR_FRAME_VP8 = 5, OCR_FRAME_J2K = 6, OCR_FRAME_J2K_CODED = 7, OCR_FRAME_TIFF_CODED = 8, OCR_FRAME_TIFF_DEFLATE = 9, OCR_FRAME_TIFF_FAX = 10 } ocr_frame_kind;
typedef struct ocr_coded_frame {
  int kind;           /* ocr_frame_kind */
  const void* frame;  /* ocr_jpeg_frame, ocr_png_frame, ocr_raw_frame, ocr_tiff_frame, ocr_webp_frame, ocr_vp8_frame, ocr_j2k_frame, ocr_j2k_coded, ocr_tiff_coded (TIFF_CODED and TIFF_DEFLATE) or ocr_tiff_fax */
} ocr_coded_frame;
int ocr_pipe_stage_batch(ocr_pipe* h, int slot, const ocr_coded_frame* frames, int count);
const char* ocr_pipe_label(ocr_pipe* h, int id);
/* network input size the detector uses for a rows x cols image (ResizeImgType0) */
int ocr_pipe_det_shape(ocr_pipe* h, int rows, int cols, int* net_rows, int* net_cols);
/* binding-cache statistics summed over the pipeline's networks: out = {network runs, runs that had to bind a new
 * shape (plan the arena, build the launch list), runs replayed from a recorded hipGraph} */
int ocr_pipe_stats(ocr_pipe* h, long long out[3]);
/* HIP-event timing of every kernel launch of the three networks during subsequent runs */
int ocr_pipe_timing(ocr_pipe* h, int enable);
/* restrict the events to launches whose name contains substr (NULL or "": all launches) */
int ocr_pipe_timing_filter(ocr_pipe* h, const char* substr);
int ocr_pipe_timing_report(ocr_pipe* h, char* buf, size_t cap);

/* Utility::GetRotateCropImage (/root/reference/src/utility.cpp:137-190) for n boxes (n x 8 ints,
 * x0,y0..x3,y3) of one host image: bounding-box crop, cv::getPerspectiveTransform onto
 * int(|p0p1|) x int(|p0p3|), cv::warpPerspective (bilinear, constant-0 border: the reference passes
 * BORDER_REPLICATE in the flags slot), and a 90-degree turn when rows >= 1.5 cols.
 * Crop k is out[out_off[k] .. out_off[k+1]) as packed BGR of out_rows[k] x out_cols[k];
 * out_off has n+1 entries.  A box whose bounding box is empty or leaves the image is an OCR_ERR_ARG
 * (the reference would throw from cv::Mat::operator() inside a noexcept function). */
int ocr_rotate_crop(const uint8_t* bgr, int rows, int cols, size_t row_stride, const int32_t* boxes, int n, uint8_t* out,
                    size_t out_cap, size_t* out_off, int* out_rows, int* out_cols);
/* size of that crop without computing it (host arithmetic only) */
int ocr_rotate_crop_shape(int rows, int cols, const int32_t* box, int* out_rows, int* out_cols);

/* The classifier's in-place rotations (/root/reference/src/ocr_worker.cpp:255-262: `cv::rotate(img_list[i], img_list[i], 1)`
 * on crops that are ROI views of ONE image, so overlapping crops see each other's result): rotates the n rectangles
 * (n x 4 ints: x, y, w, h, inside the image) of a host image by 180 degrees in list order, on the device.  Rectangles
 * that are connected through intersections form a group that keeps list order; groups run concurrently. */
int ocr_rotate180_rois(uint8_t* bgr, int rows, int cols, size_t row_stride, const int32_t* rects, int n);

/* device memory helpers for callers without a HIP binding of their own (bench, tests) */
int ocr_dev_alloc(void** p, size_t bytes);
int ocr_dev_free(void* p);
int ocr_dev_upload(void* dst, const void* src, size_t bytes);
int ocr_dev_download(void* dst, const void* src, size_t bytes);
int ocr_dev_sync(void);
/* measurement aid (decode_tool --time): *ms = the device time of ONE plain copy kernel over `bytes` (dst, src from
 * ocr_dev_alloc; 16 bytes a lane), the mean of `iters` - the yardstick a streaming kernel's time is set against in the same run */
int ocr_dev_copy_time(void* dst, const void* src, size_t bytes, int iters, double* ms);

/* ---------------------------------------------------------------- raw network taps (parity tests) */
typedef struct ocr_net ocr_net;
/* kind: "det" | "cls" | "rec".  weights: path of a .pdiparams file (NULL: <model_dir>/inference.pdiparams,
 * falling back to <model_dir>/synthetic.pdiparams). */
int ocr_net_create(const char* kind, const char* model_dir, const char* weights, int device_id, ocr_net** out);
/* the same with the stages' precision parameter ("fp32" | "fp16") */
int ocr_net_create_precision(const char* kind, const char* model_dir, const char* weights, int device_id, const char* precision,
                             ocr_net** out);
void ocr_net_destroy(ocr_net* h);
/* x: host f32 [N,H,W,3] (already normalised, BGR order).  keep_all: 0 = production launch list and arena reuse;
 * 1 = every plan tensor materialised in its own slot (no fusion); 2 = the production launch list (SE gates folded,
 * depthwise->pointwise pairs fused) with every tensor it writes kept in its own slot. */
int ocr_net_forward(ocr_net* h, const float* x, int N, int H, int W, int keep_all);
/* Ragged batch (rec only): N text lines of height H, line n of width widths[n]; x = the lines' [H][widths[n]][3]
 * blocks one after the other.  One launch list for all widths (the recognizer's production path: every batch of
 * rec_batch_num lines has its own tensor width, src/ocr_rec.cpp:47-72); each line's results are those of
 * ocr_net_forward on that line alone.  ocr_net_fetch then returns a tensor's lines one after the other with
 * dims = {1, 1, total pixels, C} (per-line vectors such as the SE gates: {N, 1, 1, C}). */
int ocr_net_forward_ragged(ocr_net* h, const float* x, int N, int H, const int* widths, int keep_all);
/* Ragged batch of IMAGES (det only): N images of their own sizes heights[n] x widths[n] (multiples of 32, what
 * ResizeImgType0 produces, src/preprocess_op.cpp:84-88) in one launch list - the detector's path for batches of mixed
 * sizes; x = the images' [h][w][3] blocks one after the other.  keep_all 0 or 2.  ocr_net_fetch returns a tensor's
 * images one after the other, dims = {1, 1, total pixels at that tensor's resolution, C}. */
int ocr_net_forward_ragged_images(ocr_net* h, const float* x, int N, const int* heights, const int* widths, int keep_all);
int ocr_net_num_tensors(ocr_net* h);
/* 1 if the last forward wrote tensor `tid` to device memory (fused-away tensors never exist), else 0 */
int ocr_net_tensor_exists(ocr_net* h, int tid);
/* tid < 0: network output.  out receives logical NHWC; dims = {N,H,W,C}. */
int ocr_net_fetch(ocr_net* h, int tid, float* out, size_t cap_floats, int dims[4]);
/* HIP-event timing of the launches of subsequent ocr_net_forward calls */
int ocr_net_timing(ocr_net* h, int enable);
/* writes "name ms count flops bytes\n" lines */
int ocr_net_timing_report(ocr_net* h, char* buf, size_t cap);

/* ---------------------------------------------------------------- server networks (BASELINE configs[4]) - raw taps
 * "PP-OCRv4_server_det (ResNet50 backbone) + SVTR-large rec, fp16": the reference ships no such graph or weights (SURVEY.md
 * section 8d, cfg5) - the two plans (cpp-paddle-ocr_amd/plans/srv_det.plan, srv_rec.plan) are hand-written from the public
 * PaddleOCR model definitions, NOT reference artifacts; parameters are seeded (<model_dir>/synthetic.pdiparams, names and shapes
 * from the plan's parameter table).  What is matched is the reference's `precision` constructor argument
 * (/root/reference/src/ocr_det.cpp:50-57, /root/reference/include/paddle_ocr/ocr_det.h:60-89): "fp16" = f16 tensors, f16 matrix
 * instructions, f32 accumulation; "fp32" = the PARITY TWIN of the same launch list, bit-identical to the oracle's run of the
 * plan.  kind: "det" | "rec".  x: host f32 [N,H,W,3] (normalised; det: H, W multiples of 32; rec: 48 x 320).  Output tensor
 * (tid < 0): det = the probability map [N,H,W,1]; rec = the CTC logits [N,1,W/4,6625]. */
typedef struct ocr_srv_net ocr_srv_net;
int ocr_srv_net_create(const char* kind, const char* model_dir, int device_id, const char* precision, ocr_srv_net** out);
void ocr_srv_net_destroy(ocr_srv_net* h);
/* keep_all != 0: every tensor keeps its own arena slot (parity taps of intermediate tensors) */
int ocr_srv_net_forward(ocr_srv_net* h, const float* x, int N, int H, int W, int keep_all);
/* `iters` more runs on the input the last forward uploaded (timing loops) */
int ocr_srv_net_rerun(ocr_srv_net* h, int N, int H, int W, int iters);
int ocr_srv_net_num_tensors(ocr_srv_net* h);
int ocr_srv_net_fetch(ocr_srv_net* h, int tid, float* out, size_t cap_floats, int dims[4]);
/* test hooks for the CTC head: ocr_srv_net_set_ctc switches the head's partial mode as the recognizer stage does (the next forward
 * re-binds); ocr_srv_net_ctc_tail issues the tail launch the stage issues behind the network - launch_ctc_reduce on the head's
 * partials with the handle's own slot count and step (returned; 0 outside partial mode), else launch_argmax_softmax on its logits -
 * for the rows of the current binding (returned in *rows; OCR_ERR_CAPACITY when cap_rows is below it). */
int ocr_srv_net_set_ctc(ocr_srv_net* h, int on);
int ocr_srv_net_ctc_tail(ocr_srv_net* h, int32_t* amax, float* pmax, long cap_rows, long* rows, int* slots, int* step);
int ocr_srv_net_timing(ocr_srv_net* h, int enable);
int ocr_srv_net_timing_report(ocr_srv_net* h, char* buf, size_t cap);
/* test hooks on the binding the last forward made (tests/test_gpu_srv_ops.py checks every launch alone against a float64
 * reference).  ocr_srv_net_num_launches: launches of that binding.  ocr_srv_net_launch_info: launch i's name, the tensor it
 * writes and the tensors it reads (a residual and every source of a folded concat included; the pack launch reads tid 0, the
 * input).  ocr_srv_net_run_launches: launches [first, first + count) enqueued alone (on the input the last forward uploaded)
 * and waited for.  ocr_srv_net_upload: caller data, logical NHWC f32 of the tensor's element count, written into tensor `tid`
 * as its element type (f16 / f32), pad channels zero.  A launch's output never shares arena bytes with its inputs. */
int ocr_srv_net_num_launches(ocr_srv_net* h);
int ocr_srv_net_launch_info(ocr_srv_net* h, int i, char* name, size_t name_cap, int* out_tid, int* in_tids, int in_cap, int* n_in);
int ocr_srv_net_run_launches(ocr_srv_net* h, int first, int count);
int ocr_srv_net_upload(ocr_srv_net* h, int tid, const float* data, size_t count);
/* test taps for the GEMM family alone (tests/test_gpu_srv_gemm.py).  ocr_srv_net_create_plan: as ocr_srv_net_create on the CALLER's
 * plan text and .pdiparams file (records = the plan's `# param` names in sorted order); a plan that does not parse or reads a
 * tensor before it is written is OCR_ERR_ARG, a missing parameter OCR_ERR_MODEL.  ocr_srv_net_set_config: every GEMM launch of the
 * handle on tile configuration `cfg` (-1: the default choice - OCR_SRV_CFG, the tune file, the heuristic or the timing loop - which
 * also holds while nothing is set); the next forward re-binds.  strict != 0: a launch the configuration cannot run fails that
 * forward with OCR_ERR_ARG and a message (op index, configuration name, the dispatch's reason) instead of falling back; the handle
 * stays usable.  An id that names no configuration is OCR_ERR_ARG.  ocr_srv_gemm_*: the configuration table, read-only - ids run
 * 0 .. num_configs - 1, an unused id has name NULL and column width 0. */
int ocr_srv_net_create_plan(const char* plan_text, const char* params_path, int device_id, const char* precision, ocr_srv_net** out);
int ocr_srv_net_set_config(ocr_srv_net* h, int cfg, int strict);
int ocr_srv_gemm_num_configs(void);
const char* ocr_srv_gemm_config_name(int cfg);
int ocr_srv_gemm_config_bn(int cfg);

/* self-tests / fault injection (tests): ocr_selftest_refuse_launch - a network launch whose name contains `substr` is
 * refused as if its launcher had rejected the shape (NULL or "" switches it off): the run must fail with OCR_ERR_DEVICE
 * and a message, never abort.  ocr_selftest_lds_memo - the per-device dynamic-LDS attribute memo of the kernel
 * launchers exercised on faked device indices (no HIP call: runs without a GPU). */
int ocr_selftest_refuse_launch(const char* substr);
int ocr_selftest_lds_memo(void);

/* The device's ClipperOffset / UnClip alone, for vectors held OUTSIDE the library (tests/golden/unclip_ref*: outputs of the
 * reference's own compiled src/clipper.cpp) - the one place where the HIP code can face the reference itself.
 * ocr_selftest_unclip: ClipperOffset(jtRound, etClosedPolygon).AddPath(quad).Execute(delta) as DBPostProcessor::UnClip
 * calls it (/root/reference/src/postprocess_op.cpp:46-55, /root/reference/src/clipper.cpp:3779-4021) for n quads
 * (n x 8 int32: x0,y0..x3,y3) and their deltas; out: n x cap x 2 int64 (X, Y of the solution path), counts[n] = its vertex
 * count (0: Execute returned no path; -1: more than the kernel's 512-vertex scratch); trig (may be NULL): n x 3 doubles, the
 * round join's steps, m_sin, m_cos as the device's math library computes them (clipper.cpp:3800-3818), before any rounding.
 * ocr_selftest_unclip_box: the whole UnClip -> cv::minAreaRect -> GetMiniBoxes of one candidate
 * (/root/reference/src/postprocess_op.cpp:39-72,134-168) for n boxes (n x 8 float, GetMiniBoxes order) at one unclip ratio;
 * out14 per box: RotatedRect (cx, cy, w, h, angle), ssid, four corners (x, y); status per box: {POST_ERR bit or 0,
 * vertices of the offset polygon}. */
int ocr_selftest_unclip(const int32_t* quads, const double* deltas, int n, int64_t* out, int cap, int* counts, double* trig);
int ocr_selftest_unclip_box(const float* boxes, float unclip_ratio, int n, float* out14, int* status);

/* Stage tap of the detector's post-processing (tests/test_gpu_post_stages.py): what the launch sequence of the last
 * ocr_det_post on this handle left in its device buffers - nothing is launched, nothing computed again on the device.
 * The caller sets the three capacities and the pointers; the call sets rows .. nverts (also when it answers OCR_ERR_CAPACITY,
 * so that the caller can size its buffers) and fills:
 *   bitmap      rows*cols bytes {0,1}: the map the kernels read (after the 2x2 dilate with use_dilation)
 *   ncont_all   borders discovered; ncont = min(ncont_all, 1000) borders kept, in cv::findContours' order
 *   starts      per kept border the pixel (y*cols + x) its raster scan met first: the border's first pixel for an outer border,
 *               the background pixel right of it for a hole border
 *   npts        per kept border its CHAIN_APPROX_SIMPLE vertex count
 *   voff, verts per kept border the first (x, y) pair of its npts vertices in verts, or -1: borders of one or two vertices are
 *               dropped before anything is stored.  Vertices come in the order the key pool holds them after the call: contour
 *               order with det_db_score_mode "slow", and with "fast" for borders of at most 512 vertices (sorted in LDS; a
 *               longer border was sorted in place and comes back ordered by (x, y))
 *   cand_valid, cand_boxes   per kept border whether it gave a box, and the box (8 int32) if so
 *   record      per kept border OCR_POST_REC_FLOATS floats written by the per-border kernel itself: the four GetMiniBoxes
 *               corners (x, y) of the contour's min-area rectangle, [8] its ssid, [9] the box score, [10] the number of mask
 *               pixels the score averaged over; what a candidate did not reach holds OCR_POST_REC_FILL (as bits)
 * The first call on a handle switches the record on for the ocr_det_post calls that follow and is refused (OCR_ERR_ARG), as
 * is every call that has no recorded ocr_det_post before it; NULL pointers: OCR_ERR_ARG; a capacity too small:
 * OCR_ERR_CAPACITY.  The handle stays usable after every refusal. */
#define OCR_POST_REC_FLOATS 12
#define OCR_POST_REC_FILL 0xFFFFFFFFu
typedef struct ocr_post_stages {
  size_t cap_pixels; /* in: bytes of bitmap */
  int cap_borders;   /* in: entries of starts / npts / voff / cand_valid, cand_boxes / 8, record / OCR_POST_REC_FLOATS */
  int cap_verts;     /* in: (x, y) pairs of verts */
  uint8_t* bitmap;
  int32_t *starts, *npts, *voff, *verts, *cand_valid, *cand_boxes;
  float* record;
  int rows, cols, ncont_all, ncont, nverts; /* out */
} ocr_post_stages;
int ocr_det_post_stages(ocr_det* h, ocr_post_stages* out);

/* The resize-and-normalise launches of csrc/kernels_pre.hip alone (tests/test_gpu_pre_ops.py), each with the named stage's own
 * normalisation table.  Every output buffer is pre-filled on the device with the byte OCR_SELFTEST_FILL and comes back with
 * OCR_SELFTEST_GUARD more bytes than the launch may write, taken from device memory right behind its last element: what no
 * descriptor names, guard included, must still hold the fill.  Arguments the launchers do not define are refused with
 * OCR_ERR_ARG before anything reaches the device.
 * ocr_selftest_det_pre: launch_det_pre (detector table) on the device copy of buf[buf_bytes]; image i starts at byte src_offset +
 * i * src_image_bytes of that copy (the copy itself is 256-byte aligned, so src_offset % 4 is the alignment of the first
 * image), rows src_stride apart.  out: N*dh*dw*3 floats + guard, resized: N*dh*dw*3 bytes + guard.
 * ocr_selftest_line_pre: launch_line_pre on ROIs of one parent image (rows x cols BGR, rows stride apart, rows*stride bytes);
 * lines: n x 6 int32 (x, y, w, h, resize_w, slot), slots distinct and < nslots; pad_mode OCR_PAD_REC (byte 0 before
 * normalising) | OCR_PAD_CLS (0.0f after); stage OCR_STAGE_REC | OCR_STAGE_CLS.  out: nslots*imgH*imgW*3 floats + guard.
 * ocr_selftest_line_pre_ragged: launch_line_pre_ragged (the recognizer's pad); lines: n x 6 int32 (x, y, w, h, resize_w,
 * tensor_w), line i at pixel imgH * (tensor widths before it).  out: imgH * sum(tensor_w) * 3 floats + guard. */
#define OCR_SELFTEST_FILL 0xA5
#define OCR_SELFTEST_GUARD 256
#define OCR_PAD_REC 0
#define OCR_PAD_CLS 1
#define OCR_STAGE_REC 1
#define OCR_STAGE_CLS 2
int ocr_selftest_det_pre(const uint8_t* buf, size_t buf_bytes, size_t src_offset, size_t src_stride, size_t src_image_bytes, int N,
                         int sh, int sw, int dh, int dw, float* out, uint8_t* resized);
int ocr_selftest_line_pre(const uint8_t* img, int rows, int cols, size_t stride, const int32_t* lines, int n, int imgH, int imgW,
                          int nslots, int pad_mode, int stage, float* out);
int ocr_selftest_line_pre_ragged(const uint8_t* img, int rows, int cols, size_t stride, const int32_t* lines, int n, int imgH,
                                 int stage, float* out);

/* The crop geometry between detector and recognizer alone (tests/test_gpu_crop_ops.py, tests/test_crop_ref.py).  Arguments
 * the launchers do not define are refused with OCR_ERR_ARG before anything reaches the device.
 * ocr_selftest_warp_crops: ONE launch_warp_crops over n descriptors on the device copy of src[src_bytes].  The CALLER gives the
 * matrix (destination -> source, as the kernel reads it), the column block bw0 and max_pixels (what sizes the grid; at least
 * one); crop k reads the sw x sh pixels that start at byte src_off of the copy, rows sstride apart (they must lie inside it),
 * and writes dw * dh * 3 bytes at out_off[k] of an output of out_bytes bytes.  The device output is pre-filled with
 * OCR_SELFTEST_FILL; out receives all of it and OCR_SELFTEST_GUARD more bytes from behind its last.
 * ocr_selftest_rotate180_groups: ONE launch_rotate180_groups on the device copy of buf[buf_bytes], which comes back whole.
 * rois: n x 6 int64 (byte offset of the view's first pixel, row stride, x, y, w, h; every ROI inside the buffer), already in
 * launch order; seg: ngroups + 1 ascending offsets into rois, seg[0] = 0, as the caller chooses them (ngroups = 0: nothing
 * is launched).  ROIs of DIFFERENT groups that could touch one byte are refused: the launch leaves their order open.
 * ocr_selftest_crop_plan (host only): every field of the plan of Utility::GetRotateCropImage for one box of a rows x cols
 * image - fields = {left, top, sw, sh, dw, dh, rot, orows, ocols, bw0}, minv = the 9 doubles of the inverse homography;
 * OCR_ERR_ARG where ocr_rotate_crop refuses the box.
 * ocr_selftest_rotation_groups (host only): the grouping ocr_rotate180_rois and the pipeline launch with, for n rectangles
 * (n x 4 int32: x, y, w, h) of which rectangle i lies in view views[i]: order[n] = request indices group after group,
 * seg[*ngroups + 1] = the groups' offsets into order (seg has room for n + 1). */
typedef struct ocr_warp_case {
  uint64_t src_off, sstride;
  int32_t sw, sh, dw, dh, rot, bw0;
  double m[9];
} ocr_warp_case;
int ocr_selftest_warp_crops(const uint8_t* src, size_t src_bytes, const ocr_warp_case* cases, int n, int max_pixels,
                            const uint64_t* out_off, size_t out_bytes, uint8_t* out);
int ocr_selftest_rotate180_groups(uint8_t* buf, size_t buf_bytes, const int64_t* rois, int n, const int32_t* seg, int ngroups);
int ocr_selftest_crop_plan(int rows, int cols, const int32_t* box8, int32_t* fields, double* minv);
int ocr_selftest_rotation_groups(const int32_t* rects, const int32_t* views, int n, int32_t* order, int32_t* seg, int* ngroups);

/* The recognizer's tail launches alone, on caller-held data (tests/test_gpu_rec_tail.py): what turns logits into (arg max,
 * probability) per CTC step and steps into characters.  Each calls the launch function production binds.  Every output is
 * pre-filled with OCR_SELFTEST_FILL and comes back with OCR_SELFTEST_GUARD more bytes, taken from behind its last element
 * (so every output buffer holds count * 4 + OCR_SELFTEST_GUARD bytes); what a launcher does not define is refused with
 * OCR_ERR_ARG before anything reaches the device.
 * ocr_selftest_softmax_argmax: launch_softmax_argmax (the mobile heads' unfused form) on rows x C logits, C <= 8192; probs
 * (rows * C, may be NULL), amax, pmax (rows each).
 * ocr_selftest_head_combine: launch_head_combine (second half of the mobile fused head) on rows x groups partials (group
 * maximum, group sum, index of the group's first maximum).
 * ocr_selftest_srv_argmax: srv::launch_argmax_softmax on rows of C logits ld floats apart (rows * ld floats are uploaded);
 * one_pass: the f16 build's form (ld % 4 == 0 and ld >= C rounded up to 4), else the two-pass form.
 * ocr_selftest_ctc_reduce: srv::launch_ctc_reduce on rows x slots partials of 4 floats (maximum, sum of exp(x - maximum), the
 * first maximum's column as int bits, unused); slots 0, step, 2 step, .. are folded.
 * ocr_selftest_ctc: the greedy collapse of nsteps_total (amax, pmax) pairs.  lines NULL: launch_ctc on nlines lines of T steps
 * (nlines * T == nsteps_total); lines: nlines x 2 int32 (first step, step count) - launch_ctc_ragged; chars != 0:
 * launch_ctc_chars in either form, which also fills steps / nsteps / probs.  ids, steps, nsteps, probs: nlines * max_len; lens,
 * scores: nlines.
 * ocr_selftest_topk_lines: launch_ctc_topk on nlines lines of T rows (C f32 at `pitch` floats) each; lens[nlines], steps and p0
 * [nlines * max_len] as launch_ctc_chars leaves them; out_ids / out_probs: nlines * max_len * k. */
int ocr_selftest_softmax_argmax(const float* logits, long rows, int C, float* probs, int32_t* amax, float* pmax);
int ocr_selftest_head_combine(const float* hmax, const float* hsum, const int32_t* hidx, long rows, int groups, int32_t* amax,
                              float* pmax);
int ocr_selftest_srv_argmax(const float* logits, long rows, int C, int ld, int one_pass, int32_t* amax, float* pmax);
int ocr_selftest_ctc_reduce(const float* part, long rows, int slots, int step, int32_t* amax, float* pmax);
int ocr_selftest_ctc(const int32_t* amax, const float* pmax, long nsteps_total, int nlines, int T, const int32_t* lines, int max_len,
                     int chars, int32_t* ids, int32_t* lens, float* scores, int32_t* steps, int32_t* nsteps, float* probs);
int ocr_selftest_topk_lines(const float* rows, int nlines, int T, int C, int pitch, const int32_t* lens, const int32_t* steps,
                            const float* p0, int max_len, int k, int32_t* out_ids, float* out_probs);

/* The mobile recognizer's head alone, through the network's own binder: the embedded rec plan with the weights file `weights`
 * (NULL: model_dir's), bound on `lines` blank lines of imgH x imgW with the head's sinks set as the recognizer stage sets them;
 * rows (nrows x K f32, nrows = lines * the CTC steps of such a line) replace the head linear's input and the binding's last two
 * launches run alone - the fused head (mode 0), the unfused one with the logits kept (1) or with probabilities requested (2).
 * amax / pmax: nrows values + OCR_SELFTEST_GUARD bytes; logits (modes 1, 2): nrows * *ncols; names: the two launches' names and `logits_stored` or
 * `logits_fused` (whether the binder folded the softmax into the linear), separated by newlines. */
int ocr_selftest_rec_head(const char* model_dir, const char* weights, const char* precision, const float* rows, long nrows, int K,
                          int lines, int imgH, int imgW, int mode, int32_t* amax, float* pmax, float* logits, int* ncols, char* names,
                          size_t names_cap);

/* numerics probe (tests): out[8*n] = a/b, sqrt|a|, ocr_expf(a), fma(a,b,a), a*b+a, rint(a*log2e), hswish(a), hswish(b) */
int ocr_probe(const float* a, const float* b, float* out, int n);

#ifdef __cplusplus
}
#endif
#endif /* OCR_HIP_H_ */
