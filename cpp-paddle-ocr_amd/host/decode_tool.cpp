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
// decode_tool --stage <model dir> <jpeg file> <out.ppm> [...]: all files as ONE batch through ocr_pipe_stage_jpeg_frames
// into a pipeline's staging slot, each staged image read back (ocr_pipe_slot_image) and written.  With a PNG among the
// files the batch goes through ocr_pipe_stage_coded, with a BMP or PNM among them through ocr_pipe_stage_frames.
// decode_tool --time <iters> <jpeg file>: device time of that pixel half's two kernels (HIP events around `iters`
// launches each, ocr_jpeg_time / ocr_jpeg_time_frame), one JSON line.
// decode_tool --time <iters> <png file> [<batch>]: the same for a PNG (ocr_png_time: upload of the inflated stream, pixel
// stage); with <batch> > 1 that many copies of the file as one batch (ocr_png_time_batch), times per batch.
// decode_tool --time <iters> <bmp or pnm file> [<batch>]: the same for a BMP / PNM (ocr_raw_time / ocr_raw_time_batch: upload
// of the stored rows, pixel stage), and "host_pixels_ms": raw::pixels of the same frame(s) on one host thread, the stage
// the device stage would replace.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "ocr_ipc_service.h"

static int time_device(int iters, const char* in, int batch) {
  std::vector<uint8_t> bytes;
  PaddleOCR::Image im;
  if (PaddleOCR::ipc::read_file(in, bytes) && bytes.size() > 8 && bytes[0] == 0x89 && bytes[1] == 'P') {
    auto f = std::make_shared<PaddleOCR::png::Frame>();
    if (!PaddleOCR::png::parse(bytes.data(), bytes.size(), *f)) { fprintf(stderr, "decode failed\n"); return 1; }
    im.rows = f->height; im.cols = f->width;
    im.png = f;
    const ocr_png_frame d = im.png_frame();
    std::vector<const ocr_png_frame*> all((size_t)(batch > 1 ? batch : 1), &d);
    double ms[2];
    if ((batch > 1 ? ocr_png_time_batch(all.data(), (int)all.size(), 0, iters, ms) : ocr_png_time(&d, 0, iters, ms)) != OCR_OK) { fprintf(stderr, "device timing failed: %s\n", ocr_last_error()); return 1; }
    printf("{\"size\": [%d, %d], \"color_type\": %d, \"bit_depth\": %d, \"interlace\": %d, \"segments\": %d, \"batch\": %d, \"iters\": %d, "
           "\"upload_ms\": %.5f, \"pixel_stage_ms\": %.5f}\n", d.height, d.width, d.color_type, d.bit_depth, d.interlace, d.nsegments, (int)all.size(), iters, ms[0], ms[1]);
    return 0;
  }
  if (bytes.size() > 2 && ((bytes[0] == 'B' && bytes[1] == 'M') || (bytes[0] == 'P' && bytes[1] >= '1' && bytes[1] <= '6'))) {
    auto f = std::make_shared<PaddleOCR::raw::Frame>();
    if (!PaddleOCR::raw::parse(bytes.data(), bytes.size(), *f)) { fprintf(stderr, "decode failed\n"); return 1; }
    im.rows = f->height; im.cols = f->width;
    im.raw = f;
    const ocr_raw_frame d = im.raw_frame();
    std::vector<const ocr_raw_frame*> all((size_t)(batch > 1 ? batch : 1), &d);
    double ms[2];
    if ((batch > 1 ? ocr_raw_time_batch(all.data(), (int)all.size(), 0, iters, ms) : ocr_raw_time(&d, 0, iters, ms)) != OCR_OK) { fprintf(stderr, "device timing failed: %s\n", ocr_last_error()); return 1; }
    std::vector<uint8_t> px;
    const auto t0 = std::chrono::steady_clock::now();
    for (int i = 0; i < iters; ++i)
      for (size_t k = 0; k < all.size(); ++k) PaddleOCR::raw::pixels(*f, px);
    const double host_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() / iters;
    printf("{\"size\": [%d, %d], \"kind\": %d, \"bottom_up\": %d, \"batch\": %d, \"iters\": %d, \"upload_ms\": %.5f, \"pixel_stage_ms\": %.5f, "
           "\"host_pixels_ms\": %.5f}\n", d.height, d.width, d.kind, d.bottom_up, (int)all.size(), iters, ms[0], ms[1], host_ms);
    return 0;
  }
  if (bytes.empty() || !PaddleOCR::ipc::decode_jpeg(bytes, im, true) || !im.device_decodable()) { fprintf(stderr, "decode failed\n"); return 1; }
  const ocr_jpeg_frame d = im.jpeg_frame();
  double ms[2];
  int rc;
  if (im.needs_frame()) rc = ocr_jpeg_time_frame(&d, 0, iters, ms);
  else { const ocr_jpeg_img o = im.jpeg_desc(); rc = ocr_jpeg_time(&o, 0, iters, ms); }
  if (rc != OCR_OK) { fprintf(stderr, "device timing failed: %s\n", ocr_last_error()); return 1; }
  printf("{\"stored\": [%d, %d], \"orientation\": %d, \"iters\": %d, \"idct_ms\": %.5f, \"pixel_stage_ms\": %.5f}\n",
         d.rows, d.cols, d.orientation, iters, ms[0], ms[1]);
  return 0;
}

static void write_ppm(FILE* f, const uint8_t* bgr, int rows, int cols) {
  fprintf(f, "P6\n%d %d\n255\n", cols, rows);
  for (size_t p = 0; p < (size_t)rows * cols; ++p) { const uint8_t rgb[3] = {bgr[3 * p + 2], bgr[3 * p + 1], bgr[3 * p]}; fwrite(rgb, 1, 3, f); }
}

static int stage_batch(const std::string& model_dir, int n, char** pairs) {
  std::vector<PaddleOCR::Image> ims((size_t)n);
  std::vector<ocr_jpeg_frame> frames((size_t)n);
  std::vector<ocr_png_frame> pframes((size_t)n);
  std::vector<const ocr_jpeg_frame*> jp((size_t)n, nullptr);
  std::vector<const ocr_png_frame*> pp((size_t)n, nullptr);
  std::vector<ocr_raw_frame> rframes((size_t)n);
  std::vector<const ocr_raw_frame*> rp((size_t)n, nullptr);
  bool coded = false, with_raw = false;
  for (int i = 0; i < n; ++i) {
    std::vector<uint8_t> bytes;
    if (!PaddleOCR::ipc::read_file(pairs[2 * i], bytes) || !PaddleOCR::ipc::decode_image(bytes, ims[i], true, true) || !ims[i].device_decodable()) {
      fprintf(stderr, "decode failed: %s\n", pairs[2 * i]);
      return 1;
    }
    if (ims[i].raw) { rframes[i] = ims[i].raw_frame(); rp[i] = &rframes[i]; coded = with_raw = true; }
    else if (ims[i].png) { pframes[i] = ims[i].png_frame(); pp[i] = &pframes[i]; coded = true; }
    else { frames[i] = ims[i].jpeg_frame(); jp[i] = &frames[i]; }
  }
  const std::string det = model_dir + "/det", cls = model_dir + "/cls", rec = model_dir + "/rec", dict = rec + "/ppocr_keys_v1.txt";
  ocr_pipe_cfg c;
  ocr_pipe_cfg_default(&c);
  c.det.model_dir = det.c_str(); c.cls.model_dir = cls.c_str(); c.rec.model_dir = rec.c_str(); c.rec.label_path = dict.c_str();
  ocr_pipe* pipe = nullptr;
  if (ocr_pipe_create(&c, &pipe) != OCR_OK) { fprintf(stderr, "pipeline: %s\n", ocr_last_error()); return 1; }
  int rc = 0;
  if ((with_raw ? ocr_pipe_stage_frames(pipe, 0, jp.data(), pp.data(), rp.data(), n) : coded ? ocr_pipe_stage_coded(pipe, 0, jp.data(), pp.data(), n) : ocr_pipe_stage_jpeg_frames(pipe, 0, frames.data(), n)) != OCR_OK) { fprintf(stderr, "staging failed: %s\n", ocr_last_error()); rc = 1; }
  for (int i = 0; i < n && !rc; ++i) {
    std::vector<uint8_t> px((size_t)ims[i].rows * ims[i].cols * 3);
    int rows = 0, cols = 0;
    if (ocr_pipe_slot_image(pipe, 0, i, px.data(), px.size(), &rows, &cols) != OCR_OK || rows != ims[i].rows || cols != ims[i].cols) {
      fprintf(stderr, "read-back failed: %s: %s\n", pairs[2 * i], ocr_last_error());
      rc = 1;
      break;
    }
    FILE* f = fopen(pairs[2 * i + 1], "wb");
    if (!f) { rc = 1; break; }
    write_ppm(f, px.data(), rows, cols);
    fclose(f);
  }
  ocr_pipe_destroy(pipe);
  return rc;
}

static int decode_one(bool device, bool frame, const char* in, const char* outp) {
  std::vector<uint8_t> bytes;
  PaddleOCR::Image im;
  if (!PaddleOCR::ipc::read_file(in, bytes) || !PaddleOCR::ipc::decode_image(bytes, im, device, device) || im.empty()) { fprintf(stderr, "decode failed: %s\n", in); return 1; }
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
    if (frame || im.needs_frame()) rc = ocr_jpeg_decode_frame(&d, 0, im.pixels.data(), im.pixels.size());
    else { const ocr_jpeg_img o = im.jpeg_desc(); rc = ocr_jpeg_decode(&o, 0, im.pixels.data(), im.pixels.size()); }
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
  if (argc >= 5 && !strcmp(argv[1], "--stage") && (argc - 3) % 2 == 0) return stage_batch(argv[2], (argc - 3) / 2, argv + 3);
  const bool frame = argc > 1 && !strcmp(argv[1], "--frame");
  const bool device = frame || (argc > 1 && !strcmp(argv[1], "--device"));
  const int first = device ? 2 : 1;
  if (argc - first < 2 || (argc - first) % 2) { fprintf(stderr, "usage: decode_tool [--device | --frame] <in> <out.ppm> [<in> <out.ppm> ...]\n"); return 2; }
  for (int i = first; i < argc; i += 2)
    if (int rc = decode_one(device, frame, argv[i], argv[i + 1])) return rc;
  return 0;
}
