// decode_tool [--device | --frame] <image file> <out.ppm> [<image file> <out.ppm> ...]: runs the IPC service's image
// decoders (test aid; several pairs share one process, the first failure ends it).  --device: a JPEG's
// pixel half (IDCT, upsampling, colour conversion, EXIF orientation) runs on the GPU instead of on the host - through
// ocr_jpeg_decode when ocr_jpeg_img can hold the file, else through ocr_jpeg_decode_frame.  --frame: the same, always
// through ocr_jpeg_decode_frame.
// A PNG's pixel half (unfiltering, conversion, Adam7 placement) runs on the GPU with --device / --frame too, through
// ocr_png_decode (whatever OCR_DEVICE_PNG says; a file beyond the device stage's bounds stays on the host); without them
// on the host (png_decode.h).
// A BMP's or PNM's pixel half (bit / nibble / palette expansion, 5-5-5 / 5-6-5, high bytes, row and channel order) runs
// on the GPU with --device / --frame as well, through ocr_raw_decode (whatever OCR_DEVICE_RAW says); without them on the
// host (raw_decode.h).
// decode_tool --stage <model dir> <image file> <out.ppm> [...]: all files (JPEG, PNG, BMP, PNM in any mix) as ONE batch
// through ocr_pipe_stage_frames into a pipeline's staging slot, each staged image read back (ocr_pipe_slot_image) and written.
// A "--" between pairs starts a further batch: the batches go through the same slot of the same pipeline, one after the other.
// Per batch one JSON line on stdout, "kinds": the ocr_frame_kind each file is staged as.
// decode_tool --stage-ways <model dir> <jpeg file> <out.ppm> <jpeg file> <out.ppm> [...]: one batch of JPEGs that ocr_jpeg_img
// can hold through each of ocr_pipe_stage_jpeg, _jpeg_frames, _coded and _frames; after each, the same batch with an unsound
// second image must be refused with OCR_ERR_ARG, and the slot is read back after that: <out.ppm>.jpeg, .jpeg_frames, .coded, .frames.
// decode_tool --time <iters> <jpeg file>: device time of that pixel half's two kernels (HIP events around `iters`
// launches each, ocr_jpeg_time / ocr_jpeg_time_frame), one JSON line.
// decode_tool --time <iters> <png file> [<batch>]: the same for a PNG (ocr_png_time: upload of the inflated stream, pixel
// stage); with <batch> > 1 that many copies of the file as one batch (ocr_png_time_batch), times per batch.
// decode_tool --time <iters> <bmp or pnm file> [<batch>]: the same for a BMP / PNM (ocr_raw_time / ocr_raw_time_batch: upload
// of the stored rows, pixel stage), and "host_pixels_ms": raw::pixels of the same frame(s) on one host thread, the stage
// the device stage would replace.
// A TIFF's pixel half (predictor, tile placement, planar to chunky, bit expansion, palette, 16 -> 8 bits, CMYK, alpha) runs on
// the GPU with --device / --frame too, through ocr_tiff_decode (whatever OCR_DEVICE_TIFF says); --stage takes TIFFs in the mix
// (ocr_pipe_stage_batch).  The coded route - the chunks' LZW / PackBits expansion on the device too, ocr_tiff_decode_coded - is
// taken by --device / --frame / --stage when OCR_DEVICE_TIFF=2, and by --stage for an input written "coded:<file>" whatever
// the switch says; --time measures both routes in one run: "coded_upload_ms", "expand_stage_ms", "coded_pixel_stage_ms"
// (ocr_tiff_time_coded / _batch), "coded_bytes", "host_scan_ms_per_image" (tiff::coded_fault: the extent scans, which both
// routes pay) and "host_expand_ms_per_image" (tiff::expand on one host thread, which the coded route saves).
// A Deflate TIFF goes coded under OCR_DEVICE_TIFF=3 (--device / --frame / --stage: ocr_tiff_decode_deflate,
// OCR_FRAME_TIFF_DEFLATE) and by --stage for "coded:<file>"; --time on such a file adds "coded_upload_ms", "inflate_stage_ms"
// (the inflate launch with the read-back of its counts), "coded_pixel_stage_ms" (ocr_tiff_time_deflate / _batch) and
// "host_inflate_ms_per_image" (tiff::inflate_all: zlib on one host thread).
// A CCITT fax TIFF (Compression 2, 3, 4, 32771) goes coded under OCR_DEVICE_TIFF=4 (--device / --frame / --stage:
// ocr_tiff_decode_fax, OCR_FRAME_TIFF_FAX) and by --stage for "coded:<file>"; --time on such a file adds "coded_upload_ms",
// "unfax_stage_ms", "coded_pixel_stage_ms" (ocr_tiff_time_fax / _batch), "host_scan_ms_per_image" (tiff::fax_fault: the walk of
// every stream, which both routes pay) and "host_unfax_ms_per_image" (tiff::unfax_all on one host thread, which the coded
// route saves).
// --time <iters> <tiff file> [<batch>]: ocr_tiff_time / ocr_tiff_time_batch (upload of the expanded
// chunks, pixel stage), "host_pixels_ms" (tiff::pixels on one host thread), "bytes_in" / "bytes_out" (what the kernel reads and
// writes) and "copy_ms": a plain copy kernel that reads and writes as many bytes in all (ocr_dev_copy_time), timed in the same run.
// decode_tool --stage-frames <model dir> ...: as --stage, through ocr_pipe_stage_frames (the three-array entry point: no TIFFs).
// A lossless WebP's pixel half (the inverse transforms: predictor, cross-colour, add-green, palette) runs on the GPU with
// --device / --frame too, through ocr_webp_decode (whatever OCR_DEVICE_WEBP says; a file outside the device stage's scope stays
// on the host); --stage takes WebPs in the mix; --time <iters> <webp file> [<batch>]: ocr_webp_time / ocr_webp_time_batch (upload
// of the coded data, pixel stage), "host_pixels_ms" (webp::pixels on one host thread), "bytes_in" / "bytes_out".
// A JPEG 2000 file takes the same switches: --device / --frame through ocr_j2k_decode (a file outside the device stage's scope
// stays on the host), --stage in the mix, --time through ocr_j2k_time / ocr_j2k_time_batch ("host_pixels_ms": j2k::pixels on one
// host thread, "host_tier1_ms_per_image": j2k::parse, which is what bounds a request).  The coded route - tier-1 on the device
// too, ocr_j2k_decode_coded - is taken by --device / --frame / --stage when OCR_DEVICE_J2K=2, and by --stage for an input
// written "coded:<file>" whatever the switch says (so that one batch can mix both forms); --time measures both routes in one
// run: "coded_upload_ms", "tier1_stage_ms", "coded_pixel_stage_ms" (ocr_j2k_time_coded / _batch), "coded_descriptor_bytes"
// (what one image uploads that way) and "host_tier2_ms_per_image" (j2k::parse_coded: what stays on the host).
// A lossy WebP takes the same switches: --device / --frame through ocr_vp8_decode, --stage in the mix, --time through
// ocr_vp8_time / ocr_vp8_time_batch ("host_pixels_ms": vp8::pixels on one host thread, "descriptor_bytes": what one image uploads).
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "ocr_ipc_service.h"

// ocr_jpeg_img, the first descriptor (grey and YCbCr 4:4:4 / 4:2:2 / 4:2:0: jpeg::Coefs::classic()), kept as ABI: --device and
// --time go on exercising its entry points for the files it can hold
static ocr_jpeg_img jpeg_desc(const PaddleOCR::jpeg::Coefs& j) {
  ocr_jpeg_img d;
  memset(&d, 0, sizeof d);
  d.rows = j.rows; d.cols = j.cols; d.ncomp = j.ncomp; d.hmax = j.hmax; d.vmax = j.vmax; d.orientation = j.orientation;
  for (int i = 0; i < j.ncomp; ++i) {
    const auto& c = j.comp[i];
    d.comp[i].coef = c.coef.data();
    memcpy(d.comp[i].quant, c.quant, sizeof c.quant);
    d.comp[i].bw = c.bw; d.comp[i].bh = c.bh; d.comp[i].dw = c.dw; d.comp[i].dh = c.dh;
  }
  return d;
}

// --time: `n` copies of the descriptor `d` as one batch through ocr_X_time_batch (n == 1: through ocr_X_time) into ms, then,
// where host_ms is given, pixels() - the format's stage on one host thread - for as many frames, per repetition.  false
// after reporting a failure.
template <class D, class Pixels = void (*)()>
static bool time_copies(const D& d, int n, int iters, int (*one)(const D*, int, int, double*), int (*many)(const D* const*, int, int, int, double*),
                        double* ms, Pixels pixels = nullptr, double* host_ms = nullptr) {
  const std::vector<const D*> all((size_t)n, &d);
  if ((n > 1 ? many(all.data(), n, 0, iters, ms) : one(&d, 0, iters, ms)) != OCR_OK) { fprintf(stderr, "device timing failed: %s\n", ocr_last_error()); return false; }
  if (!host_ms) return true;
  const auto t0 = std::chrono::steady_clock::now();
  for (int i = 0; i < iters; ++i)
    for (int k = 0; k < n; ++k) pixels();
  *host_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() / iters;
  return true;
}

static int time_device(int iters, const char* in, int batch) {
  const int n = batch > 1 ? batch : 1;
  std::vector<uint8_t> bytes;
  PaddleOCR::Image im;
  if (PaddleOCR::ipc::read_file(in, bytes) && bytes.size() > 8 && bytes[0] == 0x89 && bytes[1] == 'P') {
    auto f = std::make_shared<PaddleOCR::png::Frame>();
    if (!PaddleOCR::png::parse(bytes.data(), bytes.size(), *f)) { fprintf(stderr, "decode failed\n"); return 1; }
    im.rows = f->height; im.cols = f->width;
    im.png = f;
    const ocr_png_frame d = im.png_frame();
    double ms[2];
    if (!time_copies(d, n, iters, ocr_png_time, ocr_png_time_batch, ms)) return 1;
    printf("{\"size\": [%d, %d], \"color_type\": %d, \"bit_depth\": %d, \"interlace\": %d, \"segments\": %d, \"batch\": %d, \"iters\": %d, "
           "\"upload_ms\": %.5f, \"pixel_stage_ms\": %.5f}\n", d.height, d.width, d.color_type, d.bit_depth, d.interlace, d.nsegments, n, iters, ms[0], ms[1]);
    return 0;
  }
  if (PaddleOCR::ipc::is_j2k(bytes.data(), bytes.size())) {
    auto v = std::make_shared<PaddleOCR::j2k::Frame>();
    const auto p0 = std::chrono::steady_clock::now();
    if (!PaddleOCR::j2k::parse(bytes.data(), bytes.size(), *v) || !v->device_ok) { fprintf(stderr, "decode failed: %s\n", v->error ? v->error : "outside the device stage's scope"); return 1; }
    const double parse_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - p0).count();
    im.rows = v->height; im.cols = v->width;
    im.j2k = v;
    const ocr_j2k_frame d = im.j2k_frame();
    double ms[2], host_ms;
    std::vector<uint8_t> px;
    if (!time_copies(d, n, iters, ocr_j2k_time, ocr_j2k_time_batch, ms, [&] { PaddleOCR::j2k::pixels(*v, px); }, &host_ms)) return 1;
    // the coded route
    auto c = std::make_shared<PaddleOCR::j2k::Coded>();
    const auto c0 = std::chrono::steady_clock::now();
    if (!PaddleOCR::j2k::parse_coded(bytes.data(), bytes.size(), *c)) { fprintf(stderr, "decode failed: %s\n", c->frame.error ? c->frame.error : "tier-2"); return 1; }
    const double tier2_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - c0).count();
    im.j2k_coded = c;
    const ocr_j2k_coded cd = im.j2k_coded_frame();
    double cms[3];
    if (!time_copies(cd, n, iters, ocr_j2k_time_coded, ocr_j2k_time_coded_batch, cms)) return 1;
    printf("{\"size\": [%d, %d], \"j2k\": true, \"transform\": \"%s\", \"levels\": %d, \"batch\": %d, \"iters\": %d, "
           "\"upload_ms\": %.5f, \"pixel_stage_ms\": %.5f, \"host_pixels_ms\": %.5f, \"host_tier1_ms_per_image\": %.5f, \"descriptor_bytes\": %zu, \"bytes_out\": %zu, "
           "\"coded_upload_ms\": %.5f, \"tier1_stage_ms\": %.5f, \"coded_pixel_stage_ms\": %.5f, \"coded_descriptor_bytes\": %zu, \"code_blocks\": %zu, "
           "\"host_tier2_ms_per_image\": %.5f}\n",
           d.height, d.width, d.transform ? "9/7" : "5/3", v->tcs[0].levels, n, iters, ms[0], ms[1], host_ms, parse_ms,
           v->coeffs.size() * 4 + v->steps.size() * 4 + v->tcs.size() * sizeof(PaddleOCR::j2k::TileComp), (size_t)d.width * d.height * 3 * n,
           cms[0], cms[1], cms[2], c->bytes.size() + c->cblks.size() * sizeof(PaddleOCR::j2k::CodedBlock) + v->steps.size() * 4 + v->tcs.size() * sizeof(PaddleOCR::j2k::TileComp),
           c->cblks.size(), tier2_ms);
    return 0;
  }
  if (PaddleOCR::ipc::is_webp(bytes.data(), bytes.size())) {
    auto v = std::make_shared<PaddleOCR::vp8::Frame>();
    if (PaddleOCR::vp8::parse_file(bytes.data(), bytes.size(), *v)) {  // lossy
      im.rows = v->height; im.cols = v->width;
      im.vp8 = v;
      const ocr_vp8_frame d = im.vp8_frame();
      double ms[2], host_ms;
      std::vector<uint8_t> px;
      if (!time_copies(d, n, iters, ocr_vp8_time, ocr_vp8_time_batch, ms, [&] { PaddleOCR::vp8::pixels(*v, px); }, &host_ms)) return 1;
      printf("{\"size\": [%d, %d], \"lossy\": true, \"filter_type\": %d, \"batch\": %d, \"iters\": %d, "
             "\"upload_ms\": %.5f, \"pixel_stage_ms\": %.5f, \"host_pixels_ms\": %.5f, \"descriptor_bytes\": %zu, \"bytes_out\": %zu}\n",
             d.height, d.width, d.filter_type, n, iters, ms[0], ms[1], host_ms, v->mbs.size() * sizeof(PaddleOCR::vp8::Mb) + v->coeffs.size() * 2,
             (size_t)d.width * d.height * 3 * n);
      return 0;
    }
    auto f = std::make_shared<PaddleOCR::webp::Frame>();
    if (!PaddleOCR::webp::parse(bytes.data(), bytes.size(), *f) || !f->device_ok) { fprintf(stderr, "decode failed: %s\n", f->error ? f->error : "outside the device stage's scope"); return 1; }
    im.rows = f->height; im.cols = f->width;
    im.webp = f;
    const ocr_webp_frame d = im.webp_frame();
    double ms[2], host_ms;
    std::vector<uint8_t> px;
    if (!time_copies(d, n, iters, ocr_webp_time, ocr_webp_time_batch, ms, [&] { PaddleOCR::webp::pixels(*f, px); }, &host_ms)) return 1;
    size_t in = f->argb.size() * 4;
    std::string kinds;
    for (const auto& t : f->transforms) { in += t.data.size() * 4; kinds += (kinds.empty() ? "" : ", ") + std::to_string(t.kind); }
    printf("{\"size\": [%d, %d], \"coded_width\": %d, \"transforms\": [%s], \"batch\": %d, \"iters\": %d, "
           "\"upload_ms\": %.5f, \"pixel_stage_ms\": %.5f, \"host_pixels_ms\": %.5f, \"bytes_in\": %zu, \"bytes_out\": %zu}\n",
           d.height, d.width, PaddleOCR::webp::coded_width(*f), kinds.c_str(), n, iters, ms[0], ms[1], host_ms, in * n,
           (size_t)d.width * d.height * 3 * n);
    return 0;
  }
  if (PaddleOCR::ipc::is_tiff(bytes.data(), bytes.size())) {
    auto f = std::make_shared<PaddleOCR::tiff::Frame>();
    if (!PaddleOCR::tiff::parse(bytes.data(), bytes.size(), *f)) { fprintf(stderr, "decode failed\n"); return 1; }
    im.rows = f->height; im.cols = f->width;
    im.tiff = f;
    const ocr_tiff_frame d = im.tiff_frame();
    double ms[2], host_ms;
    std::vector<uint8_t> px;
    if (!time_copies(d, n, iters, ocr_tiff_time, ocr_tiff_time_batch, ms, [&] { PaddleOCR::tiff::pixels(*f, px); }, &host_ms)) return 1;
    // the yardstick of the same run: a plain copy kernel that reads and writes as many bytes in all as the pixel stage (chunks in, BGR out)
    const size_t in = f->data.size() * n, out = (size_t)d.width * d.height * 3 * n, half = (in + out) / 2;
    double copy_ms = -1;
    void *a = nullptr, *b = nullptr;
    if (ocr_dev_alloc(&a, half) == OCR_OK && ocr_dev_alloc(&b, half) == OCR_OK) {
      std::vector<uint8_t> zero(half);
      ocr_dev_upload(a, zero.data(), half);
      copy_ms = 0;
      if (ocr_dev_copy_time(b, a, half, iters, &copy_ms) != OCR_OK) copy_ms = -1;
    }
    if (a) ocr_dev_free(a);
    if (b) ocr_dev_free(b);
    printf("{\"size\": [%d, %d], \"photometric\": %d, \"bits\": %d, \"samples\": %d, \"planar\": %d, \"predictor\": %d, \"tile\": [%d, %d], \"batch\": %d, \"iters\": %d, "
           "\"upload_ms\": %.5f, \"pixel_stage_ms\": %.5f, \"host_pixels_ms\": %.5f, \"bytes_in\": %zu, \"bytes_out\": %zu, \"copy_ms\": %.5f",
           d.height, d.width, d.photometric, d.bits_per_sample, d.samples_per_pixel, d.planar, d.predictor, d.tile_width, d.tile_height, n, iters,
           ms[0], ms[1], host_ms, in, out, copy_ms);
    // the coded route (Compression 1, LZW, PackBits): upload of the coded chunks, expansion and pixel stage on the device, and
    // what the host pays either way, per image on one thread: the extent scan (both routes) and tiff::expand (the =1 route)
    auto c = std::make_shared<PaddleOCR::tiff::Coded>();
    if (PaddleOCR::tiff::parse_coded(bytes.data(), bytes.size(), *c) == PaddleOCR::tiff::kCoded && c->frame.device_ok) {
      im.tiff_coded = c;
      const ocr_tiff_coded cd = im.tiff_coded_frame();
      double cms[3];
      if (!time_copies(cd, n, iters, ocr_tiff_time_coded, ocr_tiff_time_coded_batch, cms)) return 1;
      PaddleOCR::tiff::Geometry g;
      const int reps = iters < 3 ? 3 : iters;
      auto t1 = std::chrono::steady_clock::now();
      bool sound = true;
      for (int i = 0; i < reps; ++i) sound = sound && !PaddleOCR::tiff::coded_fault(*c, g);
      const double scan_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count() / reps;
      PaddleOCR::tiff::Frame ef;
      t1 = std::chrono::steady_clock::now();
      for (int i = 0; i < reps; ++i) sound = sound && PaddleOCR::tiff::expand(*c, ef);
      const double expand_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count() / reps;
      if (!sound) { fprintf(stderr, "host expansion failed\n"); return 1; }
      printf(", \"compression\": %d, \"chunks\": %zu, \"coded_bytes\": %zu, \"coded_upload_ms\": %.5f, \"expand_stage_ms\": %.5f, \"coded_pixel_stage_ms\": %.5f, "
             "\"host_scan_ms_per_image\": %.5f, \"host_expand_ms_per_image\": %.5f",
             c->compression, c->chunks.size(), c->bytes.size(), cms[0], cms[1], cms[2], scan_ms, expand_ms);
    } else if (PaddleOCR::tiff::parse_fax(bytes.data(), bytes.size(), *c) && c->frame.device_ok && c->frame.tile_width <= PaddleOCR::tiff::kMaxFaxDeviceWidth) {
      // the fax route: upload of the coded chunks, the fax expansion and the pixel stage on the device, against the walk of
      // every stream (both routes) and tiff::unfax_all (the =1 route) per image on one host thread
      im.tiff_fax = c;
      const ocr_tiff_fax cd = im.tiff_fax_frame();
      double cms[3];
      if (!time_copies(cd, n, iters, ocr_tiff_time_fax, ocr_tiff_time_fax_batch, cms)) return 1;
      PaddleOCR::tiff::Geometry g;
      const int reps = iters < 3 ? 3 : iters;
      auto t1 = std::chrono::steady_clock::now();
      bool sound = true;
      for (int i = 0; i < reps; ++i) sound = sound && !PaddleOCR::tiff::fax_fault(*c, g);
      const double scan_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count() / reps;
      PaddleOCR::tiff::Frame ef;
      t1 = std::chrono::steady_clock::now();
      for (int i = 0; i < reps; ++i) sound = sound && PaddleOCR::tiff::unfax_all(*c, ef);
      const double unfax_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count() / reps;
      if (!sound) { fprintf(stderr, "host expansion failed\n"); return 1; }
      printf(", \"compression\": %d, \"chunks\": %zu, \"coded_bytes\": %zu, \"coded_upload_ms\": %.5f, \"unfax_stage_ms\": %.5f, \"coded_pixel_stage_ms\": %.5f, "
             "\"host_scan_ms_per_image\": %.5f, \"host_unfax_ms_per_image\": %.5f",
             c->compression, c->chunks.size(), c->bytes.size(), cms[0], cms[1], cms[2], scan_ms, unfax_ms);
    } else if (PaddleOCR::tiff::parse_deflate(bytes.data(), bytes.size(), *c) && c->frame.device_ok) {
      // the Deflate route: upload of the coded chunks, the inflate launch with its read-back and the pixel stage on the device,
      // against tiff::inflate_all - zlib on one thread - per image
      im.tiff_deflate = c;
      const ocr_tiff_coded cd = im.tiff_deflate_frame();
      double cms[3];
      if (!time_copies(cd, n, iters, ocr_tiff_time_deflate, ocr_tiff_time_deflate_batch, cms)) return 1;
      const int reps = iters < 3 ? 3 : iters;
      PaddleOCR::tiff::Frame ef;
      bool sound = true;
      const auto t1 = std::chrono::steady_clock::now();
      for (int i = 0; i < reps; ++i) sound = sound && PaddleOCR::tiff::inflate_all(*c, ef);
      const double inflate_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count() / reps;
      if (!sound) { fprintf(stderr, "host expansion failed\n"); return 1; }
      printf(", \"compression\": %d, \"chunks\": %zu, \"coded_bytes\": %zu, \"coded_upload_ms\": %.5f, \"inflate_stage_ms\": %.5f, \"coded_pixel_stage_ms\": %.5f, "
             "\"host_inflate_ms_per_image\": %.5f",
             c->compression, c->chunks.size(), c->bytes.size(), cms[0], cms[1], cms[2], inflate_ms);
    }
    printf("}\n");
    return 0;
  }
  if (bytes.size() > 2 && ((bytes[0] == 'B' && bytes[1] == 'M') || (bytes[0] == 'P' && bytes[1] >= '1' && bytes[1] <= '6'))) {
    auto f = std::make_shared<PaddleOCR::raw::Frame>();
    if (!PaddleOCR::raw::parse(bytes.data(), bytes.size(), *f)) { fprintf(stderr, "decode failed\n"); return 1; }
    im.rows = f->height; im.cols = f->width;
    im.raw = f;
    const ocr_raw_frame d = im.raw_frame();
    double ms[2], host_ms;
    std::vector<uint8_t> px;
    if (!time_copies(d, n, iters, ocr_raw_time, ocr_raw_time_batch, ms, [&] { PaddleOCR::raw::pixels(*f, px); }, &host_ms)) return 1;
    printf("{\"size\": [%d, %d], \"kind\": %d, \"bottom_up\": %d, \"batch\": %d, \"iters\": %d, \"upload_ms\": %.5f, \"pixel_stage_ms\": %.5f, "
           "\"host_pixels_ms\": %.5f}\n", d.height, d.width, d.kind, d.bottom_up, n, iters, ms[0], ms[1], host_ms);
    return 0;
  }
  if (bytes.empty() || !PaddleOCR::ipc::decode_jpeg(bytes, im, true) || !im.device_decodable()) { fprintf(stderr, "decode failed\n"); return 1; }
  const ocr_jpeg_frame d = im.jpeg_frame();
  double ms[2];
  int rc;
  if (!im.jpeg->classic()) rc = ocr_jpeg_time_frame(&d, 0, iters, ms);
  else { const ocr_jpeg_img o = jpeg_desc(*im.jpeg); rc = ocr_jpeg_time(&o, 0, iters, ms); }
  if (rc != OCR_OK) { fprintf(stderr, "device timing failed: %s\n", ocr_last_error()); return 1; }
  printf("{\"stored\": [%d, %d], \"orientation\": %d, \"iters\": %d, \"idct_ms\": %.5f, \"pixel_stage_ms\": %.5f}\n",
         d.rows, d.cols, d.orientation, iters, ms[0], ms[1]);
  return 0;
}

static void write_ppm(FILE* f, const uint8_t* bgr, int rows, int cols) {
  fprintf(f, "P6\n%d %d\n255\n", cols, rows);
  for (size_t p = 0; p < (size_t)rows * cols; ++p) { const uint8_t rgb[3] = {bgr[3 * p + 2], bgr[3 * p + 1], bgr[3 * p]}; fwrite(rgb, 1, 3, f); }
}

// one batch of --stage / --stage-ways: the files as device-decodable images, their descriptors, where the staged pixels go
struct Batch {
  std::vector<PaddleOCR::Image> ims;
  std::vector<std::string> in, out;
  PaddleOCR::DeviceFrames frames;
};

// the batch through one of the four staging entry points (way 0..3: ocr_pipe_stage_jpeg, _jpeg_frames, _coded, _frames; the first
// three take JPEGs only, the first those ocr_jpeg_img can hold).  spoil: the second image's first component loses its blocks
static int stage_way(ocr_pipe* pipe, int way, const Batch& b, bool spoil) {
  const int n = (int)b.ims.size();
  if (way == 0) {
    std::vector<ocr_jpeg_img> d;
    for (const auto& im : b.ims) d.push_back(jpeg_desc(*im.jpeg));
    if (spoil) d[1].comp[0].bw = 0;
    return ocr_pipe_stage_jpeg(pipe, 0, d.data(), n);
  }
  std::vector<ocr_jpeg_frame> d(b.frames.jf.begin(), b.frames.jf.end());
  if (spoil) d[1].comp[0].bw = 0;
  if (way == 1) return ocr_pipe_stage_jpeg_frames(pipe, 0, d.data(), n);
  std::vector<const ocr_jpeg_frame*> p;
  for (const auto& f : d) p.push_back(&f);
  return way == 2 ? ocr_pipe_stage_coded(pipe, 0, p.data(), nullptr, n) : ocr_pipe_stage_frames(pipe, 0, p.data(), nullptr, nullptr, n);
}

static int read_back(ocr_pipe* pipe, const Batch& b, const std::string& suffix) {
  for (size_t i = 0; i < b.ims.size(); ++i) {
    std::vector<uint8_t> px((size_t)b.ims[i].rows * b.ims[i].cols * 3);
    int rows = 0, cols = 0;
    if (ocr_pipe_slot_image(pipe, 0, (int)i, px.data(), px.size(), &rows, &cols) != OCR_OK || rows != b.ims[i].rows || cols != b.ims[i].cols) {
      fprintf(stderr, "read-back failed: %s: %s\n", b.in[i].c_str(), ocr_last_error());
      return 1;
    }
    FILE* f = fopen((b.out[i] + suffix).c_str(), "wb");
    if (!f) return 1;
    write_ppm(f, px.data(), rows, cols);
    fclose(f);
  }
  return 0;
}

// the batch through ocr_pipe_stage_frames, the entry point of three arrays (JPEG, PNG and raw frames only)
static int stage_three_arrays(ocr_pipe* pipe, const Batch& b) {
  const size_t n = b.frames.list.size();
  std::vector<const ocr_jpeg_frame*> jp(n, nullptr);
  std::vector<const ocr_png_frame*> pp(n, nullptr);
  std::vector<const ocr_raw_frame*> rp(n, nullptr);
  for (size_t i = 0; i < n; ++i) {
    const ocr_coded_frame& f = b.frames.list[i];
    if (f.kind == OCR_FRAME_JPEG) jp[i] = (const ocr_jpeg_frame*)f.frame;
    else if (f.kind == OCR_FRAME_PNG) pp[i] = (const ocr_png_frame*)f.frame;
    else if (f.kind == OCR_FRAME_RAW) rp[i] = (const ocr_raw_frame*)f.frame;
  }
  return ocr_pipe_stage_frames(pipe, 0, jp.data(), pp.data(), rp.data(), (int)n);
}

static int stage_batches(const std::string& model_dir, int nargs, char** args, bool ways, bool three_arrays = false) {
  std::vector<Batch> batches(1);
  for (int a = 0; a < nargs; ++a) {
    if (!strcmp(args[a], "--")) { batches.emplace_back(); continue; }
    if (a + 1 >= nargs) { fprintf(stderr, "an input without an output: %s\n", args[a]); return 2; }
    Batch& b = batches.back();
    b.in.push_back(args[a]);
    b.out.push_back(args[++a]);
  }
  for (Batch& b : batches) {
    if (b.in.empty() || (ways && (batches.size() != 1 || b.in.size() < 2))) { fprintf(stderr, "empty batch (--stage-ways: one batch of two files or more)\n"); return 2; }
    b.ims.resize(b.in.size());
    for (size_t i = 0; i < b.in.size(); ++i) {
      std::vector<uint8_t> bytes;
      if (!b.in[i].compare(0, 6, "coded:")) {  // a JPEG 2000 or TIFF file in the coded form, whatever OCR_DEVICE_J2K / OCR_DEVICE_TIFF say
        if (PaddleOCR::ipc::read_file(b.in[i].substr(6), bytes) && PaddleOCR::ipc::is_tiff(bytes.data(), bytes.size())) {
          auto t = std::make_shared<PaddleOCR::tiff::Coded>();
          const PaddleOCR::tiff::Route route = PaddleOCR::tiff::parse_coded(bytes.data(), bytes.size(), *t);
          if (route == PaddleOCR::tiff::kOtherRoute && PaddleOCR::tiff::parse_deflate(bytes.data(), bytes.size(), *t) && t->frame.device_ok) {  // OCR_FRAME_TIFF_DEFLATE
            b.ims[i].rows = t->frame.height; b.ims[i].cols = t->frame.width;
            b.ims[i].tiff_deflate = t;
            b.frames.add(b.ims[i]);
            continue;
          }
          if (route == PaddleOCR::tiff::kFaxRoute && PaddleOCR::tiff::parse_fax(bytes.data(), bytes.size(), *t) && t->frame.device_ok &&
              t->frame.tile_width <= PaddleOCR::tiff::kMaxFaxDeviceWidth) {  // OCR_FRAME_TIFF_FAX
            b.ims[i].rows = t->frame.height; b.ims[i].cols = t->frame.width;
            b.ims[i].tiff_fax = t;
            b.frames.add(b.ims[i]);
            continue;
          }
          if (route != PaddleOCR::tiff::kCoded || !t->frame.device_ok) {
            fprintf(stderr, "decode failed: %s\n", b.in[i].c_str());
            return 1;
          }
          b.ims[i].rows = t->frame.height; b.ims[i].cols = t->frame.width;
          b.ims[i].tiff_coded = t;
          b.frames.add(b.ims[i]);
          continue;
        }
        auto c = std::make_shared<PaddleOCR::j2k::Coded>();
        if (!PaddleOCR::ipc::read_file(b.in[i].substr(6), bytes) || !PaddleOCR::j2k::parse_coded(bytes.data(), bytes.size(), *c) || !c->frame.device_ok) {
          fprintf(stderr, "decode failed: %s\n", b.in[i].c_str());
          return 1;
        }
        b.ims[i].rows = c->frame.height; b.ims[i].cols = c->frame.width;
        b.ims[i].j2k_coded = c;
        b.frames.add(b.ims[i]);
        continue;
      }
      if (!PaddleOCR::ipc::read_file(b.in[i], bytes) || !PaddleOCR::ipc::decode_image(bytes, b.ims[i], true, true) || !b.ims[i].device_decodable() ||
          (ways && !(b.ims[i].jpeg && b.ims[i].jpeg->classic()))) {
        fprintf(stderr, "decode failed: %s\n", b.in[i].c_str());
        return 1;
      }
      b.frames.add(b.ims[i]);
    }
    printf("{\"kinds\": [");  // the ocr_frame_kind each file of the batch is staged as
    for (size_t i = 0; i < b.frames.list.size(); ++i) printf("%s%d", i ? ", " : "", b.frames.list[i].kind);
    printf("]}\n");
  }
  const std::string det = model_dir + "/det", cls = model_dir + "/cls", rec = model_dir + "/rec", dict = rec + "/ppocr_keys_v1.txt";
  ocr_pipe_cfg c;
  ocr_pipe_cfg_default(&c);
  c.det.model_dir = det.c_str(); c.cls.model_dir = cls.c_str(); c.rec.model_dir = rec.c_str(); c.rec.label_path = dict.c_str();
  ocr_pipe* pipe = nullptr;
  if (ocr_pipe_create(&c, &pipe) != OCR_OK) { fprintf(stderr, "pipeline: %s\n", ocr_last_error()); return 1; }
  int rc = 0;
  if (ways) {
    static const char* const name[4] = {".jpeg", ".jpeg_frames", ".coded", ".frames"};
    for (int w = 0; w < 4 && !rc; ++w) {
      if (stage_way(pipe, w, batches[0], false) != OCR_OK) { fprintf(stderr, "staging failed (%s): %s\n", name[w] + 1, ocr_last_error()); rc = 1; break; }
      const int refused = stage_way(pipe, w, batches[0], true);
      if (refused != OCR_ERR_ARG) { fprintf(stderr, "the spoilt batch was not refused with OCR_ERR_ARG (%s): %d\n", name[w] + 1, refused); rc = 1; break; }
      rc = read_back(pipe, batches[0], name[w]);  // after the refused call: the slot still holds the batch staged before it
    }
  } else {
    for (const Batch& b : batches) {
      if ((three_arrays ? stage_three_arrays(pipe, b) : b.frames.stage(pipe, 0)) != OCR_OK) { fprintf(stderr, "staging failed: %s\n", ocr_last_error()); rc = 1; }
      if (!rc) rc = read_back(pipe, b, "");
      if (rc) break;
    }
  }
  ocr_pipe_destroy(pipe);
  return rc;
}

static int decode_one(bool device, bool frame, const char* in, const char* outp) {
  std::vector<uint8_t> bytes;
  PaddleOCR::Image im;
  if (!PaddleOCR::ipc::read_file(in, bytes) || !PaddleOCR::ipc::decode_image(bytes, im, device, device) || im.empty()) { fprintf(stderr, "decode failed: %s\n", in); return 1; }
  if (im.device_decodable() && im.tiff_deflate) {
    const ocr_tiff_coded d = im.tiff_deflate_frame();
    im.pixels.resize((size_t)d.frame.height * d.frame.width * 3);
    if (ocr_tiff_decode_deflate(&d, 0, im.pixels.data(), im.pixels.size()) != OCR_OK) { fprintf(stderr, "device decode failed: %s: %s\n", in, ocr_last_error()); return 1; }
  } else
  if (im.device_decodable() && im.tiff_fax) {
    const ocr_tiff_fax d = im.tiff_fax_frame();
    im.pixels.resize((size_t)d.coded.frame.height * d.coded.frame.width * 3);
    if (ocr_tiff_decode_fax(&d, 0, im.pixels.data(), im.pixels.size()) != OCR_OK) { fprintf(stderr, "device decode failed: %s: %s\n", in, ocr_last_error()); return 1; }
  } else
  if (im.device_decodable() && im.tiff_coded) {
    const ocr_tiff_coded d = im.tiff_coded_frame();
    im.pixels.resize((size_t)d.frame.height * d.frame.width * 3);
    if (ocr_tiff_decode_coded(&d, 0, im.pixels.data(), im.pixels.size()) != OCR_OK) { fprintf(stderr, "device decode failed: %s: %s\n", in, ocr_last_error()); return 1; }
  } else
  if (im.device_decodable() && im.j2k_coded) {
    const ocr_j2k_coded d = im.j2k_coded_frame();
    im.pixels.resize((size_t)d.frame.height * d.frame.width * 3);
    if (ocr_j2k_decode_coded(&d, 0, im.pixels.data(), im.pixels.size()) != OCR_OK) { fprintf(stderr, "device decode failed: %s: %s\n", in, ocr_last_error()); return 1; }
  } else
  if (im.device_decodable() && im.j2k) {
    const ocr_j2k_frame d = im.j2k_frame();
    im.pixels.resize((size_t)d.height * d.width * 3);
    if (ocr_j2k_decode(&d, 0, im.pixels.data(), im.pixels.size()) != OCR_OK) { fprintf(stderr, "device decode failed: %s: %s\n", in, ocr_last_error()); return 1; }
  } else
  if (im.device_decodable() && im.vp8) {
    const ocr_vp8_frame d = im.vp8_frame();
    im.pixels.resize((size_t)d.height * d.width * 3);
    if (ocr_vp8_decode(&d, 0, im.pixels.data(), im.pixels.size()) != OCR_OK) { fprintf(stderr, "device decode failed: %s: %s\n", in, ocr_last_error()); return 1; }
  } else
  if (im.device_decodable() && im.webp) {
    const ocr_webp_frame d = im.webp_frame();
    im.pixels.resize((size_t)d.height * d.width * 3);
    if (ocr_webp_decode(&d, 0, im.pixels.data(), im.pixels.size()) != OCR_OK) { fprintf(stderr, "device decode failed: %s: %s\n", in, ocr_last_error()); return 1; }
  } else
  if (im.device_decodable() && im.tiff) {
    const ocr_tiff_frame d = im.tiff_frame();
    im.pixels.resize((size_t)d.height * d.width * 3);
    if (ocr_tiff_decode(&d, 0, im.pixels.data(), im.pixels.size()) != OCR_OK) { fprintf(stderr, "device decode failed: %s: %s\n", in, ocr_last_error()); return 1; }
  } else
  if (im.device_decodable() && im.raw) {
    const ocr_raw_frame d = im.raw_frame();
    im.pixels.resize((size_t)d.height * d.width * 3);
    if (ocr_raw_decode(&d, 0, im.pixels.data(), im.pixels.size()) != OCR_OK) { fprintf(stderr, "device decode failed: %s: %s\n", in, ocr_last_error()); return 1; }
  } else
  if (im.device_decodable() && im.png) {
    const ocr_png_frame d = im.png_frame();
    im.pixels.resize((size_t)d.height * d.width * 3);
    if (ocr_png_decode(&d, 0, im.pixels.data(), im.pixels.size()) != OCR_OK) { fprintf(stderr, "device decode failed: %s: %s\n", in, ocr_last_error()); return 1; }
  } else
  if (im.device_decodable()) {
    const ocr_jpeg_frame d = im.jpeg_frame();
    im.pixels.resize((size_t)d.rows * d.cols * 3);
    int rc;
    if (frame || !im.jpeg->classic()) rc = ocr_jpeg_decode_frame(&d, 0, im.pixels.data(), im.pixels.size());
    else { const ocr_jpeg_img o = jpeg_desc(*im.jpeg); rc = ocr_jpeg_decode(&o, 0, im.pixels.data(), im.pixels.size()); }
    if (rc != OCR_OK) { fprintf(stderr, "device decode failed: %s: %s\n", in, ocr_last_error()); return 1; }
  }
  FILE* f = fopen(outp, "wb");
  if (!f) return 1;
  write_ppm(f, im.pixels.data(), im.rows, im.cols);
  fclose(f);
  return 0;
}

int main(int argc, char** argv) {
  if ((argc == 4 || argc == 5) && !strcmp(argv[1], "--time")) return time_device(atoi(argv[2]), argv[3], argc == 5 ? atoi(argv[4]) : 1);
  if (argc >= 5 && !strcmp(argv[1], "--stage-frames")) return stage_batches(argv[2], argc - 3, argv + 3, false, true);
  if (argc >= 5 && (!strcmp(argv[1], "--stage") || !strcmp(argv[1], "--stage-ways"))) return stage_batches(argv[2], argc - 3, argv + 3, argv[1][7] != 0);
  const bool frame = argc > 1 && !strcmp(argv[1], "--frame");
  const bool device = frame || (argc > 1 && !strcmp(argv[1], "--device"));
  const int first = device ? 2 : 1;
  if (argc - first < 2 || (argc - first) % 2) { fprintf(stderr, "usage: decode_tool [--device | --frame] <in> <out.ppm> [<in> <out.ppm> ...]\n"); return 2; }
  for (int i = first; i < argc; i += 2)
    if (int rc = decode_one(device, frame, argv[i], argv[i + 1])) return rc;
  return 0;
}
