// OCRIPCService for Linux: the JSON request/reply protocol of the reference's Windows named-pipe service
// (/root/reference/include/paddle_ocr/ocr_ipc_service.h:19-100, /root/reference/src/ocr_ipc_service.cpp:203-448)
// over a Unix-domain stream socket; a message (the pipe's PIPE_TYPE_MESSAGE unit) is framed as a 4-byte
// little-endian length followed by that many bytes of JSON, in both directions.
//
//   {"command":"recognize","image_path":"..."}            image file: PNG, JPEG, PNM (P1 .. P6, maxval up to 65535), BMP (1 / 4 /
//                                                         8-bit paletted, RLE8 / RLE4, 16-bit 5-5-5 / 5-6-5, 24, 32 bits)
//   {"command":"recognize","image_data":"<base64>"}       the same file contents, base64
//   {"command":"status"}    -> {"success":true,"status":"{\"running\":..,\"total_requests\":..,...}"}
//   {"command":"shutdown"}  -> {"success":true,"message":"Shutdown command received, stopping service..."}
// Replies to `recognize` are the worker's result JSON (ocr_worker.cpp:155-190) unchanged; every failure is
// {"success":false,"error":"..."} with the reference's messages.  Requests of 1 MiB - 1 bytes or more are
// answered with the reference's "Data too large for buffer" error (ocr_ipc_service.cpp:222-238).
//
// Differences, by necessity: the transport (socket path instead of \\.\pipe\ocr_service); replies are compact
// JSON (jsoncpp's default writer indents); cv::imread/imdecode are replaced by the decoders below - PNG with the decoder
// of png_decode.h (own container parser, zlib's inflate through dlopen, cv::imdecode's conversions; the system's libpng16
// simplified API, also through dlopen, only where libz.so.1 is missing), PNM
// and BMP with the decoder of raw_decode.h (every form cv::imdecode reads), JPEG with the decoder of jpeg_decode.h (a restatement of libjpeg's default pipeline,
// sequential and progressive, grey / YCbCr / RGB / CMYK / YCCK at every integral sampling, checked bit for bit against
// libjpeg-turbo through PIL).
// There is no CPU worker pool: cpu_workers is accepted and ignored, gpu_workers = 0 leaves `recognize`
// answering with an error (status / shutdown still work - that is what the CPU-only tests drive).
#pragma once
#include <dlfcn.h>
#include <sys/socket.h>
#include <sys/un.h>
#include <unistd.h>

#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <memory>
#include <mutex>
#include <sstream>
#include <string>
#include <thread>
#include <vector>

#include "jpeg_decode.h"
#include "paddle_ocr_hip.h"
#include "png_decode.h"
#include "raw_decode.h"
#include "tiff_decode.h"
#include "webp_decode.h"
#include "vp8_decode.h"
#include "j2k_decode.h"

namespace PaddleOCR {
namespace ipc {

// ---- minimal JSON reader: top-level object, string members (what the protocol uses) ----
struct JsonObject {
  std::vector<std::pair<std::string, std::string>> strings;  // key -> string value
  std::string get(const std::string& k, const std::string& dflt = "") const {
    for (auto& kv : strings) if (kv.first == k) return kv.second;
    return dflt;
  }
};
class JsonParser {
 public:
  explicit JsonParser(const std::string& s) : s_(s) {}
  bool parse(JsonObject& out, std::string& err) {
    ws();
    if (!eat('{')) return fail(err, "expected '{'");
    ws();
    if (eat('}')) return tail(err);
    for (;;) {
      std::string key, val;
      ws();
      if (!string(key)) return fail(err, "expected member name");
      ws();
      if (!eat(':')) return fail(err, "expected ':'");
      ws();
      if (peek() == '"') {
        if (!string(val)) return fail(err, "bad string");
        out.strings.emplace_back(key, val);
      } else if (!skip_value()) {
        return fail(err, "bad value");
      }
      ws();
      if (eat(',')) continue;
      if (eat('}')) return tail(err);
      return fail(err, "expected ',' or '}'");
    }
  }

 private:
  bool tail(std::string& err) { ws(); return i_ == s_.size() ? true : fail(err, "trailing characters"); }
  bool fail(std::string& err, const char* what) {
    std::ostringstream o;
    o << "* Line 1, Column " << (i_ + 1) << "\n  Syntax error: " << what << "\n";
    err = o.str();
    return false;
  }
  char peek() const { return i_ < s_.size() ? s_[i_] : '\0'; }
  bool eat(char c) { if (peek() == c) { ++i_; return true; } return false; }
  void ws() { while (i_ < s_.size() && (s_[i_] == ' ' || s_[i_] == '\t' || s_[i_] == '\n' || s_[i_] == '\r')) ++i_; }
  static void utf8(std::string& o, unsigned cp) {
    if (cp < 0x80) o += (char)cp;
    else if (cp < 0x800) { o += (char)(0xC0 | (cp >> 6)); o += (char)(0x80 | (cp & 0x3F)); }
    else if (cp < 0x10000) { o += (char)(0xE0 | (cp >> 12)); o += (char)(0x80 | ((cp >> 6) & 0x3F)); o += (char)(0x80 | (cp & 0x3F)); }
    else { o += (char)(0xF0 | (cp >> 18)); o += (char)(0x80 | ((cp >> 12) & 0x3F)); o += (char)(0x80 | ((cp >> 6) & 0x3F)); o += (char)(0x80 | (cp & 0x3F)); }
  }
  bool hex4(unsigned& v) {
    v = 0;
    for (int k = 0; k < 4; ++k) {
      const char c = peek();
      unsigned d;
      if (c >= '0' && c <= '9') d = c - '0'; else if (c >= 'a' && c <= 'f') d = c - 'a' + 10; else if (c >= 'A' && c <= 'F') d = c - 'A' + 10; else return false;
      v = v * 16 + d;
      ++i_;
    }
    return true;
  }
  bool string(std::string& out) {
    if (!eat('"')) return false;
    while (i_ < s_.size()) {
      const char c = s_[i_++];
      if (c == '"') return true;
      if (c != '\\') { out += c; continue; }
      if (i_ >= s_.size()) return false;
      const char e = s_[i_++];
      switch (e) {
        case '"': out += '"'; break; case '\\': out += '\\'; break; case '/': out += '/'; break;
        case 'b': out += '\b'; break; case 'f': out += '\f'; break; case 'n': out += '\n'; break;
        case 'r': out += '\r'; break; case 't': out += '\t'; break;
        case 'u': {
          unsigned cp;
          if (!hex4(cp)) return false;
          if (cp >= 0xD800 && cp <= 0xDBFF && peek() == '\\') {  // surrogate pair
            const size_t save = i_;
            unsigned lo;
            ++i_;
            if (eat('u') && hex4(lo) && lo >= 0xDC00 && lo <= 0xDFFF) cp = 0x10000 + ((cp - 0xD800) << 10) + (lo - 0xDC00);
            else i_ = save;
          }
          utf8(out, cp);
        } break;
        default: return false;
      }
    }
    return false;
  }
  bool skip_value() {  // number, literal, array or object: skipped with nesting and strings respected
    int depth = 0;
    const size_t start = i_;
    while (i_ < s_.size()) {
      const char c = s_[i_];
      if (c == '"') { std::string tmp; if (!string(tmp)) return false; continue; }
      if (c == '{' || c == '[') ++depth;
      else if (c == '}' || c == ']') { if (depth == 0) break; --depth; }
      else if (c == ',' && depth == 0) break;
      ++i_;
    }
    return i_ > start;
  }
  const std::string& s_;
  size_t i_ = 0;
};

inline void json_escape_to(std::string& o, const std::string& s) { detail::json_escape(o, s); }
inline std::string error_reply(const std::string& msg) {
  std::string o = "{\"error\":";
  json_escape_to(o, msg);
  o += ",\"success\":false}";
  return o;
}

// ---- base64 (RFC 4648, padding optional, whitespace skipped); false on a foreign character ----
inline bool base64_decode(const std::string& in, std::vector<uint8_t>& out) {
  unsigned acc = 0;
  int bits = 0;
  for (const unsigned char c : in) {
    int v;
    if (c >= 'A' && c <= 'Z') v = c - 'A'; else if (c >= 'a' && c <= 'z') v = c - 'a' + 26; else if (c >= '0' && c <= '9') v = c - '0' + 52;
    else if (c == '+') v = 62; else if (c == '/') v = 63; else if (c == '=') break;
    else if (c == '\n' || c == '\r' || c == ' ' || c == '\t') continue; else return false;
    acc = (acc << 6) | (unsigned)v;
    bits += 6;
    if (bits >= 8) { bits -= 8; out.push_back((uint8_t)((acc >> bits) & 0xFF)); }
  }
  return true;
}

// ---- image decoders: file contents -> packed BGR (what cv::imread / cv::imdecode return) ----
// Every decoder refuses headers that would make the service allocate gigabytes from a sub-megabyte request
// (the same 64 Mpixel cap as jpeg_decode.h).
constexpr long kMaxDecodedPixels = 64L << 20;
// BMP (1 / 4 / 8-bit paletted, RLE8 / RLE4, 16-bit 5-5-5 / 5-6-5, 24, 32; OS/2 and V3 .. V5 headers) and PNM (P1 .. P6,
// maxval up to 65535) as cv::imdecode(IMREAD_COLOR) returns them: raw_decode.h.  device_pixels: the caller has a GPU worker
// that can finish the image.  Whether it is asked to is OCR_DEVICE_RAW, read once: =1 stops after the container (and the
// run-length / ASCII expansion) and leaves the per-pixel conversion to the worker, =0 or unset finishes every file on this
// host thread - RAW_DEVICE_DEFAULT below, and DESIGN section 1 (f) for why.  force_device: as =1 whatever the environment
// says (decode_tool --device / --stage).
constexpr bool RAW_DEVICE_DEFAULT = false;
inline bool raw_device_enabled() {
  static const char* env = getenv("OCR_DEVICE_RAW");
  return env && env[0] ? env[0] != '0' : RAW_DEVICE_DEFAULT;
}
inline bool decode_raw(const std::vector<uint8_t>& d, Image& im, bool device_pixels, bool force_device) {
  auto f = std::make_shared<raw::Frame>();
  if (!raw::parse(d.data(), d.size(), *f)) return false;
  im.pixels.clear();
  im.rows = f->height; im.cols = f->width;
  if (device_pixels && (force_device || raw_device_enabled())) { im.raw = std::move(f); return true; }
  if (!raw::pixels(*f, im.pixels)) { im = Image(); return false; }
  return true;
}
inline bool decode_ppm(const std::vector<uint8_t>& d, Image& im, bool device_pixels = false, bool force_device = false) {
  return d.size() >= 2 && d[0] == 'P' && decode_raw(d, im, device_pixels, force_device);
}
inline bool decode_bmp(const std::vector<uint8_t>& d, Image& im, bool device_pixels = false, bool force_device = false) {
  return d.size() >= 2 && d[0] == 'B' && d[1] == 'M' && decode_raw(d, im, device_pixels, force_device);
}
// TIFF as cv::imdecode(IMREAD_COLOR) returns it (tiff_decode.h: classic TIFF, strips and tiles, uncompressed / PackBits / LZW /
// Deflate / CCITT fax - Modified Huffman, Group 3, Group 4 -, the sample forms libtiff's RGBA interface reads).  A CCITT file is
// expanded on this host thread (ccitt_decode.h) under =0 .. =3, and the expanded 1-bit frame then goes where the switch sends
// such frames; =4 is =3 and hands CCITT files within the device bounds (and at most tiff::kMaxFaxDeviceWidth pixels a chunk)
// over coded too (tiff::parse_fax, which walks every stream with the decoder's verdict: Image::tiff_fax, OCR_FRAME_TIFF_FAX).
// A damaged fax stream refuses the file under every value alike, and *why says which rule of the coding did.  device_pixels / force_device as for BMP and PNM; the switch is
// OCR_DEVICE_TIFF, read once: =1 stops after the chunks are expanded and leaves predictor, conversion and placement to the
// worker (frames within the device stage's bounds, tiff::Frame::device_ok), =2 stops before the expansion already and leaves
// the chunks' LZW / PackBits streams to the worker as well (tiff::parse_coded, which still scans every stream; Deflate files and
// frames beyond the bounds go the =1 route), =3 is =2 and hands Deflate files within the bounds over coded too (tiff::parse_deflate, the
// container alone: the device inflates the chunks and gives the verdict per stream; a batch with a faulty stream is refused at
// staging and the worker's fallback, one request per image, gives that file the host's refusal through Image::materialise),
// =0 or unset finishes every file on this host thread.
constexpr bool TIFF_DEVICE_DEFAULT = false;
inline int tiff_device_mode() {  // 0 host, 1 expanded chunks to the device, 2 coded chunks to the device, 3 Deflate chunks too, 4 fax chunks too
  static const char* env = getenv("OCR_DEVICE_TIFF");
  return env && env[0] ? (env[0] == '0' ? 0 : (env[0] == '2' || env[0] == '3' || env[0] == '4') && !env[1] ? env[0] - '0' : 1) : (TIFF_DEVICE_DEFAULT ? 1 : 0);
}
inline bool tiff_device_enabled() { return tiff_device_mode() != 0; }
inline bool is_tiff(const uint8_t* d, size_t n) {
  return n >= 4 && ((d[0] == 'I' && d[1] == 'I' && d[2] == 42 && d[3] == 0) || (d[0] == 'M' && d[1] == 'M' && d[2] == 0 && d[3] == 42));
}
inline bool decode_tiff(const std::vector<uint8_t>& d, Image& im, bool device_pixels = false, bool force_device = false, const char** why = nullptr) {
  if (!is_tiff(d.data(), d.size())) return false;
  auto f = std::make_shared<tiff::Frame>();
  bool parsed = false;
  const int mode = tiff_device_mode();
  if (device_pixels && mode >= 2) {
    auto c = std::make_shared<tiff::Coded>();
    bool deflate = false;  // the container is read once, whatever the compression; fax streams are walked once: here for =4, else by unfax_all
    const char* fax_why = nullptr;
    const tiff::Route route = tiff::parse_any(d.data(), d.size(), *c, deflate, mode >= 4, &fax_why);
    if (route == tiff::kRefused) { if (why && fax_why) *why = fax_why; return false; }
    if (deflate) {
      if (mode >= 3 && c->frame.device_ok) {
        im.pixels.clear();
        im.rows = c->frame.height; im.cols = c->frame.width;
        im.tiff_deflate = std::move(c);
        return true;
      }
      if (!tiff::inflate_all(*c, *f)) return false;  // (beyond the device bounds: the =1 route, from the container already read)
      parsed = true;
    } else
    if (route == tiff::kFaxRoute) {
      if (mode >= 4 && c->frame.device_ok && c->frame.tile_width <= tiff::kMaxFaxDeviceWidth) {
        im.pixels.clear();
        im.rows = c->frame.height; im.cols = c->frame.width;
        im.tiff_fax = std::move(c);
        return true;
      }
      if (!tiff::unfax_all(*c, *f, &fax_why)) { if (why && fax_why) *why = fax_why; return false; }  // (the =1 route, from the container already read)
      parsed = true;
    } else
    if (route == tiff::kCoded) {
      if (c->frame.device_ok) {
        im.pixels.clear();
        im.rows = c->frame.height; im.cols = c->frame.width;
        im.tiff_coded = std::move(c);
        return true;
      }
      if (!tiff::expand(*c, *f)) return false;
      parsed = true;
    }
  }
  if (!parsed) {
    const char* fax_why = nullptr;
    if (!tiff::parse(d.data(), d.size(), *f, &fax_why)) { if (why && fax_why) *why = fax_why; return false; }
  }
  im.pixels.clear();
  im.rows = f->height; im.cols = f->width;
  if (device_pixels && f->device_ok && (force_device || tiff_device_enabled())) { im.tiff = std::move(f); return true; }
  if (!tiff::pixels(*f, im.pixels)) { im = Image(); return false; }
  return true;
}
// WebP as cv::imdecode(IMREAD_COLOR) returns it: lossless (webp_decode.h: a VP8L chunk under RIFF / WEBP or in a VP8X container)
// and lossy (vp8_decode.h: a VP8 chunk, with or without ALPH; OCR_DEVICE_WEBP=1 stops after modes and tokens and leaves
// reconstruction, loop filter and conversion to the worker).  Animated files and lossy data without a key frame are refused,
// *why says so.  device_pixels / force_device as for TIFF; the switch is
// OCR_DEVICE_WEBP, read once: =1 stops after the entropy-coded image is decoded and leaves the inverse transforms to the
// worker (frames in the device stage's scope, webp::Frame::device_ok), =0 or unset finishes every file on this host thread.
constexpr bool WEBP_DEVICE_DEFAULT = false;
inline bool webp_device_enabled() {
  static const char* env = getenv("OCR_DEVICE_WEBP");
  return env && env[0] ? env[0] != '0' : WEBP_DEVICE_DEFAULT;
}
inline bool is_webp(const uint8_t* d, size_t n) { return webp::is_webp(d, n); }
inline bool decode_webp(const std::vector<uint8_t>& d, Image& im, bool device_pixels = false, bool force_device = false, const char** why = nullptr) {
  if (!is_webp(d.data(), d.size())) return false;
  auto f = std::make_shared<webp::Frame>();
  if (!webp::parse(d.data(), d.size(), *f)) {
    if (f->vp8) {  // lossy: the payload goes to the VP8 decoder
      auto v = std::make_shared<vp8::Frame>();
      if (!vp8::parse(f->vp8, f->vp8_size, *v) || (f->canvas_width && (f->canvas_width != v->width || f->canvas_height != v->height))) {
        if (why) *why = v->error;
        return false;
      }
      im.pixels.clear();
      im.rows = v->height; im.cols = v->width;
      if (device_pixels && (force_device || webp_device_enabled())) { im.vp8 = std::move(v); return true; }
      if (!vp8::pixels(*v, im.pixels)) { im = Image(); return false; }
      return true;
    }
    if (why) *why = f->error;
    return false;
  }
  im.pixels.clear();
  im.rows = f->height; im.cols = f->width;
  if (device_pixels && f->device_ok && (force_device || webp_device_enabled())) { im.webp = std::move(f); return true; }
  if (!webp::pixels(*f, im.pixels)) { im = Image(); return false; }
  return true;
}
// JPEG 2000 (a JP2 file or a bare codestream) as cv::imdecode(IMREAD_COLOR) returns it through OpenJPEG (j2k_decode.h).  What
// the decoder refuses - code-block styles, HT, POC / PPM / PPT / RGN, palettes, other colour spaces, signed or subsampled
// components - it refuses with a reason, *why.  device_pixels / force_device as for TIFF; the switch is OCR_DEVICE_J2K, read
// once: =1 stops after tier-1 and leaves dequantisation, the inverse wavelet and component transforms and the conversion to
// the worker (frames in the device stage's scope, j2k::Frame::device_ok), =2 stops after tier-2 already and leaves the code
// blocks to the worker as well (j2k::parse_coded; the same scope, other frames are finished here), =0 or unset finishes every
// file on this host thread.
constexpr bool J2K_DEVICE_DEFAULT = false;
inline int j2k_device_mode() {  // 0 host, 1 coefficients to the device, 2 coded blocks to the device
  static const char* env = getenv("OCR_DEVICE_J2K");
  return env && env[0] ? (env[0] == '0' ? 0 : env[0] == '2' && !env[1] ? 2 : 1) : (J2K_DEVICE_DEFAULT ? 1 : 0);
}
inline bool j2k_device_enabled() { return j2k_device_mode() != 0; }
inline bool is_j2k(const uint8_t* d, size_t n) { return j2k::is_j2k(d, n); }
inline bool decode_j2k(const std::vector<uint8_t>& d, Image& im, bool device_pixels = false, bool force_device = false, const char** why = nullptr) {
  if (!is_j2k(d.data(), d.size())) return false;
  auto f = std::make_shared<j2k::Frame>();
  if (device_pixels && j2k_device_mode() == 2) {
    auto c = std::make_shared<j2k::Coded>();
    if (!j2k::parse_coded(d.data(), d.size(), *c)) {
      if (why) *why = c->frame.error;
      return false;
    }
    if (c->frame.device_ok) {
      im.pixels.clear();
      im.rows = c->frame.height; im.cols = c->frame.width;
      im.j2k_coded = std::move(c);
      return true;
    }
    if (!j2k::finish_coded(*c, *f)) return false;
  } else if (!j2k::parse(d.data(), d.size(), *f)) {
    if (why) *why = f->error;
    return false;
  }
  im.pixels.clear();
  im.rows = f->height; im.cols = f->width;
  if (device_pixels && f->device_ok && (force_device || j2k_device_enabled())) { im.j2k = std::move(f); return true; }
  if (!j2k::pixels(*f, im.pixels)) { im = Image(); return false; }
  return true;
}
// libpng16 simplified API (png.h: png_image, PNG_IMAGE_VERSION 1, PNG_FORMAT_BGR = 0x12), resolved at run time
struct PngImage {
  void* opaque;
  uint32_t version, width, height, format, flags, colormap_entries, warning_or_error;
  char message[64];
};
inline bool decode_png_libpng(const std::vector<uint8_t>& d, Image& im) {
  static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
  if (d.size() < 8 || memcmp(d.data(), sig, 8)) return false;
  static void* lib = dlopen("libpng16.so.16", RTLD_NOW | RTLD_GLOBAL);
  if (!lib) return false;
  typedef int (*BeginFn)(PngImage*, const void*, size_t);
  typedef int (*FinishFn)(PngImage*, const void*, void*, int32_t, void*);
  typedef void (*FreeFn)(PngImage*);
  static BeginFn begin = (BeginFn)dlsym(lib, "png_image_begin_read_from_memory");
  static FinishFn finish = (FinishFn)dlsym(lib, "png_image_finish_read");
  static FreeFn pfree = (FreeFn)dlsym(lib, "png_image_free");
  if (!begin || !finish || !pfree) return false;
  PngImage pi;
  memset(&pi, 0, sizeof pi);
  pi.version = 1;
  if (!begin(&pi, d.data(), d.size())) return false;
  pi.format = 0x12;  // PNG_FORMAT_BGR: 8-bit, colour, blue first, alpha removed (composited on black like a
                     // missing background; cv::imread(IMREAD_COLOR) drops alpha without compositing - differs
                     // only for translucent pixels)
  if (pi.width == 0 || pi.height == 0 || pi.width > 100000 || pi.height > 100000 ||
      (long)pi.width * (long)pi.height > kMaxDecodedPixels) { pfree(&pi); return false; }
  im.rows = (int)pi.height; im.cols = (int)pi.width;
  im.pixels.resize((size_t)pi.width * pi.height * 3);
  if (!finish(&pi, nullptr, im.pixels.data(), 0, nullptr)) { pfree(&pi); im = Image(); return false; }
  return true;
}
// PNG as cv::imdecode(IMREAD_COLOR) returns it (png_decode.h: alpha dropped, high bytes of 16-bit samples, no gamma).
// device_pixels: the caller has a GPU worker that can finish the image.  Whether it is asked to is OCR_DEVICE_PNG, read
// once: =1 stops after the inflate and leaves unfiltering and conversion to the worker (frames within the device
// stage's bounds, png::Frame::device_ok; others are finished here), =0 or unset finishes every PNG on this host thread -
// PNG_DEVICE_DEFAULT below, and DESIGN section 1 (f) for why.  force_device: as =1 whatever the environment says
// (decode_tool --device / --stage).  Without libz.so.1 the libpng path above is what is left - with its differences for
// translucent, 16-bit and gamma-tagged files.
constexpr bool PNG_DEVICE_DEFAULT = false;
inline bool png_device_enabled() {
  static const char* env = getenv("OCR_DEVICE_PNG");
  return env && env[0] ? env[0] != '0' : PNG_DEVICE_DEFAULT;
}
inline bool decode_png(const std::vector<uint8_t>& d, Image& im, bool device_pixels = false, bool force_device = false) {
  static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
  if (d.size() < 8 || memcmp(d.data(), sig, 8)) return false;
  if (!png::available()) return decode_png_libpng(d, im);
  auto f = std::make_shared<png::Frame>();
  if (!png::parse(d.data(), d.size(), *f)) { im = Image(); return false; }
  im.pixels.clear();
  im.rows = f->height; im.cols = f->width;
  if (device_pixels && f->device_ok && (force_device || png_device_enabled())) { im.png = std::move(f); return true; }
  if (!png::pixels(*f, im.pixels)) { im = Image(); return false; }
  return true;
}
// device_pixels: stop after the entropy decoding and leave the pixel half to the GPU worker (OCR_DEVICE_JPEG=0 or
// device_pixels = false: everything on this host thread)
inline bool decode_jpeg(const std::vector<uint8_t>& d, Image& im, bool device_pixels = false) {
  if (d.size() < 4 || d[0] != 0xFF || d[1] != 0xD8) return false;
  jpeg::Decoder dec;
  static const char* env = getenv("OCR_DEVICE_JPEG");
  if (device_pixels && !(env && env[0] == '0')) {
    auto c = std::make_shared<jpeg::Coefs>();
    if (!dec.decode_coefficients(d.data(), d.size(), *c)) { im = Image(); return false; }
    im.pixels.clear();
    im.rows = c->out_rows(); im.cols = c->out_cols();  // the oriented size: what the device decode writes
    im.jpeg = std::move(c);
    return true;
  }
  if (!dec.decode(d.data(), d.size(), im.pixels, im.rows, im.cols)) { im = Image(); return false; }
  return true;
}
// force_device: PNG, BMP / PNM, TIFF, WebP and JPEG 2000 take the device route whatever OCR_DEVICE_PNG / OCR_DEVICE_RAW / OCR_DEVICE_TIFF /
// OCR_DEVICE_WEBP / OCR_DEVICE_J2K say (decode_tool).  why: set where a file is refused for a reason its sender should read (a lossy or
// animated WebP), left alone otherwise
inline bool decode_image(const std::vector<uint8_t>& bytes, Image& im, bool device_pixels = false, bool force_device = false, const char** why = nullptr) {
  return decode_png(bytes, im, device_pixels, force_device) || decode_jpeg(bytes, im, device_pixels) ||
         decode_ppm(bytes, im, device_pixels, force_device) || decode_bmp(bytes, im, device_pixels, force_device) ||
         decode_tiff(bytes, im, device_pixels, force_device, why) || decode_webp(bytes, im, device_pixels, force_device, why) ||
         decode_j2k(bytes, im, device_pixels, force_device, why);
}
inline bool read_file(const std::string& path, std::vector<uint8_t>& out) {
  std::ifstream f(path, std::ios::binary);
  if (!f) return false;
  out.assign(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
  return true;
}

}  // namespace ipc

class OCRIPCService {
 public:
  static const int PIPE_OUTPUT_BUFFER_SIZE = 65536;   // ocr_ipc_service.h:86
  static const int READ_BUFFER_SIZE = 1048576;        // ocr_ipc_service.h:88

  OCRIPCService(const std::string& model_dir, const std::string& socket_path = "/tmp/ocr_service.sock", int gpu_workers = 0,
                int cpu_workers = 1)
      : model_dir_(model_dir), socket_path_(socket_path), gpu_workers_(gpu_workers), cpu_workers_(cpu_workers) {}
  ~OCRIPCService() { stop(); }

  bool start() {
    if (running_) return true;
    if (gpu_workers_ > 0) {
      gpu_worker_pool_.reset(new GPUWorkerPool(model_dir_, gpu_workers_));
      gpu_worker_pool_->start();
    }
    listen_fd_ = socket(AF_UNIX, SOCK_STREAM, 0);
    if (listen_fd_ < 0) return false;
    sockaddr_un addr;
    memset(&addr, 0, sizeof addr);
    addr.sun_family = AF_UNIX;
    if (socket_path_.size() >= sizeof addr.sun_path) return false;
    strcpy(addr.sun_path, socket_path_.c_str());
    unlink(socket_path_.c_str());
    if (bind(listen_fd_, (sockaddr*)&addr, sizeof addr) != 0 || listen(listen_fd_, 16) != 0) { close(listen_fd_); listen_fd_ = -1; return false; }
    running_ = true;
    accept_thread_ = std::thread(&OCRIPCService::acceptLoop, this);
    return true;
  }
  void stop() {
    std::lock_guard<std::mutex> stop_lock(stop_mutex_);  // a second caller waits for the first to finish
    if (!running_.exchange(false)) return;
    if (listen_fd_ >= 0) { shutdown(listen_fd_, SHUT_RDWR); close(listen_fd_); listen_fd_ = -1; }
    if (accept_thread_.joinable() && accept_thread_.get_id() != std::this_thread::get_id()) accept_thread_.join();
    {
      std::lock_guard<std::mutex> lock(client_threads_mutex_);
      for (int fd : client_fds_) shutdown(fd, SHUT_RDWR);
    }
    for (;;) {  // client threads remove themselves; wait for them
      std::thread t;
      {
        std::lock_guard<std::mutex> lock(client_threads_mutex_);
        if (client_threads_.empty()) break;
        t = std::move(client_threads_.back());
        client_threads_.pop_back();
      }
      if (t.joinable()) t.join();
    }
    if (gpu_worker_pool_) gpu_worker_pool_->stop();
    unlink(socket_path_.c_str());
  }
  bool isRunning() const { return running_; }
  void waitUntilStopped() {
    while (running_) std::this_thread::sleep_for(std::chrono::milliseconds(20));
    std::lock_guard<std::mutex> stop_lock(stop_mutex_);  // ... and for whoever is stopping it to be done
  }

  // processIPCRequest (ocr_ipc_service.cpp:310-423)
  std::string processIPCRequest(const std::string& request_json) {
    try {
      ipc::JsonObject req;
      std::string errors;
      if (!ipc::JsonParser(request_json).parse(req, errors)) return ipc::error_reply("Invalid JSON: " + errors);
      const std::string command = req.get("command");
      if (command == "recognize") {
        const std::string image_path = req.get("image_path"), image_base64 = req.get("image_data");
        Image image;
        std::string error_msg;
        const char* why = nullptr;  // what a decoder has to say to the sender: a lossy or animated WebP is refused in so many words
        if (!image_path.empty()) {
          std::vector<uint8_t> bytes;
          if (!ipc::read_file(image_path, bytes) || !ipc::decode_image(bytes, image, gpu_worker_pool_ != nullptr, false, &why) || image.empty())
            error_msg = "Failed to load image from path: " + image_path;
        } else if (!image_base64.empty()) {
          std::vector<uint8_t> bytes;
          if (!ipc::base64_decode(image_base64, bytes)) error_msg = "Base64 decode error: invalid character";
          else if (!ipc::decode_image(bytes, image, gpu_worker_pool_ != nullptr, false, &why) || image.empty()) error_msg = "Failed to decode base64 image data";
        } else {
          error_msg = "Missing image_path or image_data";
        }
        if (!error_msg.empty() && why) error_msg += std::string(": ") + why;
        if (!error_msg.empty()) return ipc::error_reply(error_msg);
        if (!gpu_worker_pool_) return ipc::error_reply("No GPU workers configured (this build has no CPU path)");
        const int request_id = request_counter_.fetch_add(1);
        // a Deflate TIFF handed over coded (OCR_DEVICE_TIFF=3): nobody has looked at its streams yet
        const std::shared_ptr<tiff::Coded> deflate = image.tiff_deflate;
        auto request = std::make_shared<OCRRequest>(request_id, std::move(image));
        total_requests_.fetch_add(1);
        std::string result = gpu_worker_pool_->submitRequest(request).get();
        if (deflate && result.find("\"success\":true") == std::string::npos) {
          // the worker failed the request.  It has asked the host already where the device refused a stream (processRequest), so
          // this is about the words alone: a file zlib refuses gets the reply it gets where it fails to decode on this thread
          // (OCR_DEVICE_TIFF=0), and is not counted as a request either, as there
          tiff::Frame f;
          if (!tiff::inflate_all(*deflate, f)) {
            total_requests_.fetch_sub(1);
            return ipc::error_reply(!image_path.empty() ? "Failed to load image from path: " + image_path : "Failed to decode base64 image data");
          }
        }
        if (result.find("\"success\":true") != std::string::npos) successful_requests_.fetch_add(1);
        const size_t p = result.find("\"processing_time_ms\":");
        if (p != std::string::npos) {
          std::lock_guard<std::mutex> lock(stats_mutex_);
          total_processing_time_ += atof(result.c_str() + p + 21);
        }
        return result;
      } else if (command == "status") {
        std::string o = "{\"status\":";
        ipc::json_escape_to(o, getStatusInfo());
        o += ",\"success\":true}";
        return o;
      } else if (command == "shutdown") {
        std::thread([this]() {  // let the reply go out first (ocr_ipc_service.cpp:381-403)
          std::this_thread::sleep_for(std::chrono::milliseconds(50));
          this->stop();
        }).detach();
        return "{\"message\":\"Shutdown command received, stopping service...\",\"success\":true}";
      }
      return ipc::error_reply("Unknown command: " + command);
    } catch (const std::exception& e) {
      return ipc::error_reply(e.what());
    }
  }

  // getStatusInfo (ocr_ipc_service.cpp:438-448)
  std::string getStatusInfo() const {
    double avg = 0.0;
    {
      std::lock_guard<std::mutex> lock(stats_mutex_);
      avg = total_requests_.load() > 0 ? total_processing_time_ / total_requests_.load() : 0.0;
    }
    char buf[256];
    snprintf(buf, sizeof buf, "{\"average_processing_time_ms\":%.17g,\"running\":%s,\"successful_requests\":%d,\"total_requests\":%d}", avg,
             running_.load() ? "true" : "false", successful_requests_.load(), total_requests_.load());
    return buf;
  }

 private:
  static constexpr size_t kMaxClients = 256;
  void acceptLoop() {
    while (running_) {
      const int fd = accept(listen_fd_, nullptr, nullptr);
      if (fd < 0) { if (!running_) break; continue; }
      {
        // a bound on concurrent clients (each holds a thread and a 1 MiB request buffer): beyond it the connection is
        // closed at once, which a client sees as "service busy" and retries
        std::lock_guard<std::mutex> lock(client_threads_mutex_);
        if (client_fds_.size() >= kMaxClients) { close(fd); continue; }
      }
      const int big = 2 * READ_BUFFER_SIZE;
      setsockopt(fd, SOL_SOCKET, SO_RCVBUF, &big, sizeof big);
      setsockopt(fd, SOL_SOCKET, SO_SNDBUF, &big, sizeof big);
      std::lock_guard<std::mutex> lock(client_threads_mutex_);
      client_fds_.push_back(fd);
      client_threads_.emplace_back(&OCRIPCService::handleClientConnection, this, fd);
    }
  }
  static bool read_all(int fd, void* p, size_t n) {
    char* c = (char*)p;
    while (n) {
      const ssize_t r = recv(fd, c, n, 0);
      if (r <= 0) return false;
      c += r;
      n -= (size_t)r;
    }
    return true;
  }
  static bool write_all(int fd, const void* p, size_t n) {
    const char* c = (const char*)p;
    while (n) {
      const ssize_t r = send(fd, c, n, MSG_NOSIGNAL);
      if (r <= 0) return false;
      c += r;
      n -= (size_t)r;
    }
    return true;
  }
  // handleClientConnection (ocr_ipc_service.cpp:203-308): one message in, one message out
  void handleClientConnection(int fd) {
    std::vector<char> buffer(READ_BUFFER_SIZE);
    while (running_) {
      uint32_t len = 0;
      if (!read_all(fd, &len, 4)) break;  // peer closed
      std::string response;
      if (len >= (uint32_t)READ_BUFFER_SIZE - 1) {
        // the pipe version reads at most READ_BUFFER_SIZE - 1 bytes and rejects a message that fills them
        response = ipc::error_reply("Data too large for buffer (max 1MB). Consider using file path transmission.");
        uint32_t left = len;  // drain the oversized message so the stream stays in step
        bool ok = true;
        while (left && ok) { const uint32_t n = left < (uint32_t)READ_BUFFER_SIZE ? left : (uint32_t)READ_BUFFER_SIZE; ok = read_all(fd, buffer.data(), n); left -= n; }
        if (!ok) break;
      } else {
        if (!read_all(fd, buffer.data(), len)) break;
        response = len ? processIPCRequest(std::string(buffer.data(), (size_t)len)) : std::string();
        if (!len) continue;  // "Received 0 bytes": ignored (ocr_ipc_service.cpp:213-217)
      }
      const uint32_t rl = (uint32_t)response.size();
      if (!write_all(fd, &rl, 4) || !write_all(fd, response.data(), response.size())) break;
    }
    close(fd);
    std::lock_guard<std::mutex> lock(client_threads_mutex_);
    for (size_t i = 0; i < client_fds_.size(); ++i)
      if (client_fds_[i] == fd) { client_fds_.erase(client_fds_.begin() + i); break; }
    for (size_t i = 0; i < client_threads_.size(); ++i)
      if (client_threads_[i].get_id() == std::this_thread::get_id()) {
        client_threads_[i].detach();
        client_threads_.erase(client_threads_.begin() + i);
        break;
      }
  }

  std::string model_dir_, socket_path_;
  int gpu_workers_, cpu_workers_;
  std::atomic<bool> running_{false};
  int listen_fd_ = -1;
  std::thread accept_thread_;
  std::vector<std::thread> client_threads_;
  std::vector<int> client_fds_;
  std::mutex client_threads_mutex_, stop_mutex_;
  std::unique_ptr<GPUWorkerPool> gpu_worker_pool_;
  std::atomic<int> request_counter_{1}, total_requests_{0}, successful_requests_{0};
  mutable std::mutex stats_mutex_;
  double total_processing_time_ = 0.0;
};

}  // namespace PaddleOCR
