// decode_tool [--device] <image file> <out.ppm> [<image file> <out.ppm> ...]: runs the IPC service's image decoders
// (test aid; several pairs share one process, the first failure ends it).  --device: a JPEG's
// pixel half (IDCT, upsampling, colour conversion, EXIF orientation) runs on the GPU through ocr_jpeg_decode instead of
// on the host.
// decode_tool --time <iters> <jpeg file>: device time of that pixel half's two kernels (HIP events around `iters`
// launches each, ocr_jpeg_time), one JSON line.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "ocr_ipc_service.h"

static int time_device(int iters, const char* in) {
  std::vector<uint8_t> bytes;
  PaddleOCR::Image im;
  if (!PaddleOCR::ipc::read_file(in, bytes) || !PaddleOCR::ipc::decode_jpeg(bytes, im, true) || !im.device_decodable()) { fprintf(stderr, "decode failed\n"); return 1; }
  const ocr_jpeg_img d = im.jpeg_desc();
  double ms[2];
  if (ocr_jpeg_time(&d, 0, iters, ms) != OCR_OK) { fprintf(stderr, "device timing failed: %s\n", ocr_last_error()); return 1; }
  printf("{\"stored\": [%d, %d], \"orientation\": %d, \"iters\": %d, \"idct_ms\": %.5f, \"pixel_stage_ms\": %.5f}\n",
         d.rows, d.cols, d.orientation, iters, ms[0], ms[1]);
  return 0;
}

static int decode_one(bool device, const char* in, const char* outp) {
  std::vector<uint8_t> bytes;
  PaddleOCR::Image im;
  if (!PaddleOCR::ipc::read_file(in, bytes) || !PaddleOCR::ipc::decode_image(bytes, im, device) || im.empty()) { fprintf(stderr, "decode failed: %s\n", in); return 1; }
  if (im.device_decodable()) {
    const ocr_jpeg_img d = im.jpeg_desc();
    im.pixels.resize((size_t)d.rows * d.cols * 3);
    if (ocr_jpeg_decode(&d, 0, im.pixels.data(), im.pixels.size()) != OCR_OK) { fprintf(stderr, "device decode failed: %s: %s\n", in, ocr_last_error()); return 1; }
  }
  FILE* f = fopen(outp, "wb");
  if (!f) return 1;
  fprintf(f, "P6\n%d %d\n255\n", im.cols, im.rows);
  for (size_t p = 0; p < (size_t)im.rows * im.cols; ++p) { const uint8_t rgb[3] = {im.pixels[3 * p + 2], im.pixels[3 * p + 1], im.pixels[3 * p]}; fwrite(rgb, 1, 3, f); }
  fclose(f);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 4 && !strcmp(argv[1], "--time")) return time_device(atoi(argv[2]), argv[3]);
  const bool device = argc > 1 && !strcmp(argv[1], "--device");
  const int first = device ? 2 : 1;
  if (argc - first < 2 || (argc - first) % 2) { fprintf(stderr, "usage: decode_tool [--device] <in> <out.ppm> [<in> <out.ppm> ...]\n"); return 2; }
  for (int i = first; i < argc; i += 2)
    if (int rc = decode_one(device, argv[i], argv[i + 1])) return rc;
  return 0;
}
