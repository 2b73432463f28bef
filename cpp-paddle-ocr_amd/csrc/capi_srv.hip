// C-ABI of the server networks' raw taps (BASELINE configs[4]; include/ocr_hip.h "server networks").
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <sstream>

#include "capi_common.h"
#include "srv_net.h"

using namespace ocr;

namespace ocr {
// the parameter table of a server plan: its `# param <name> <dims>` lines (there is no .pdmodel to take names from)
static std::vector<std::string> srv_param_names(const char* plan) {
  std::vector<std::string> names;
  std::stringstream ss(plan);
  std::string line;
  while (std::getline(ss, line))
    if (line.rfind("# param ", 0) == 0) {
      std::stringstream ls(line.substr(8));
      std::string n;
      ls >> n;
      names.push_back(n);
    }
  std::sort(names.begin(), names.end());  // the order .pdiparams records are written in
  return names;
}
std::string server_arch(const std::string& model_dir) {
  if (file_exists(model_dir + "/inference.pdmodel") || file_exists(model_dir + "/model.pdmodel")) return "";
  FILE* f = fopen((model_dir + "/arch.txt").c_str(), "r");
  if (!f) return "";
  char buf[64] = {0};
  const size_t n = fread(buf, 1, sizeof buf - 1, f);
  fclose(f);
  std::string t(buf, n);
  while (!t.empty() && (t.back() == '\n' || t.back() == '\r' || t.back() == ' ')) t.pop_back();
  return (t == "srv_det" || t == "srv_rec") ? t : "";
}
bool load_server_model_dir(const std::string& model_dir, const char* kind, WeightMap& w, std::string& err) {
  const char* plan = embedded_plan(kind);
  if (!plan) { err = std::string("no server plan ") + kind; return false; }
  std::string params;
  for (const char* n : {"/inference.pdiparams", "/model.pdiparams", "/synthetic.pdiparams"})
    if (file_exists(model_dir + n)) { params = model_dir + n; break; }
  if (params.empty()) { err = "No parameter file found in " + model_dir; return false; }
  return pdiparams_read(params, srv_param_names(plan), w, err);
}
}  // namespace ocr

struct ocr_srv_net {
  SrvNet net;
  hipStream_t stream = nullptr;
  float* x_dev = nullptr;
  size_t x_cap = 0;
  int device = 0;
};

extern "C" {

int ocr_srv_net_create(const char* kind, const char* model_dir, int device_id, const char* precision, ocr_srv_net** out) {
  if (!kind || !model_dir || !out || !precision) return fail(OCR_ERR_ARG, "null argument");
  const bool half = !strcmp(precision, "fp16");
  if (!half && strcmp(precision, "fp32")) return fail(OCR_ERR_ARG, "precision must be fp16 (the mode BASELINE configs[4] names) or fp32 (the parity twin)");
  const std::string pk = std::string("srv_") + kind;
  const char* plan = embedded_plan(pk.c_str());
  if (!plan) return fail(OCR_ERR_ARG, "kind must be det or rec");
  int rc = ocr_rt_init(device_id);
  if (rc) return rc;
  WeightMap w;
  std::string err;
  if (!load_server_model_dir(model_dir, pk.c_str(), w, err)) return fail(OCR_ERR_MODEL, err);
  std::unique_ptr<ocr_srv_net> h(new ocr_srv_net());
  h->device = device_id;
  if (!h->net.load(plan, w, half, err)) return fail(OCR_ERR_MODEL, err);
  CAPI_HIP(g_stream_create(&h->stream));
  *out = h.release();
  return OCR_OK;
}

// test tap (tests/test_gpu_srv_gemm.py): ocr_srv_net_create on the CALLER's plan text and parameter file - the plan's `# param` lines
// name the records of the .pdiparams file (tools/synth_weights.py writes that format), in sorted order
int ocr_srv_net_create_plan(const char* plan_text, const char* params_path, int device_id, const char* precision, ocr_srv_net** out) {
  if (!plan_text || !params_path || !out || !precision) return fail(OCR_ERR_ARG, "null argument");
  const bool half = !strcmp(precision, "fp16");
  if (!half && strcmp(precision, "fp32")) return fail(OCR_ERR_ARG, "precision must be fp16 or fp32 (the parity twin)");
  int rc = ocr_rt_init(device_id);
  if (rc) return rc;
  WeightMap w;
  std::string err;
  if (!file_exists(params_path)) return fail(OCR_ERR_MODEL, std::string("No parameter file ") + params_path);
  if (!pdiparams_read(params_path, srv_param_names(plan_text), w, err)) return fail(OCR_ERR_MODEL, err);
  std::unique_ptr<ocr_srv_net> h(new ocr_srv_net());
  h->device = device_id;
  if (!h->net.load(plan_text, w, half, err)) return fail(err.rfind("server plan:", 0) == 0 ? OCR_ERR_ARG : OCR_ERR_MODEL, err);
  CAPI_HIP(g_stream_create(&h->stream));
  *out = h.release();
  return OCR_OK;
}

// test tap: SrvNet::set_config - every GEMM launch of this handle on tile configuration `cfg` (-1: the default choice again)
int ocr_srv_net_set_config(ocr_srv_net* h, int cfg, int strict) {
  if (!h) return fail(OCR_ERR_ARG, "null handle");
  if (cfg < -1 || cfg >= srv::gemm_num_configs() || (cfg >= 0 && srv::gemm_config_bn(cfg) == 0)) return fail(OCR_ERR_ARG, "no such tile configuration: " + std::to_string(cfg));
  h->net.set_config(cfg, strict != 0);
  return OCR_OK;
}
int ocr_srv_gemm_num_configs(void) { return srv::gemm_num_configs(); }
const char* ocr_srv_gemm_config_name(int cfg) { return cfg >= 0 && cfg < srv::gemm_num_configs() && srv::gemm_config_bn(cfg) ? srv::gemm_config_name(cfg) : nullptr; }
int ocr_srv_gemm_config_bn(int cfg) { return cfg >= 0 && cfg < srv::gemm_num_configs() ? srv::gemm_config_bn(cfg) : 0; }

void ocr_srv_net_destroy(ocr_srv_net* h) {
  if (!h) return;
  (void)rt_set_device(h->device);
  if (h->x_dev) (void)g_free(h->x_dev);
  if (h->stream) (void)hipStreamDestroy(h->stream);
  delete h;
}

int ocr_srv_net_forward(ocr_srv_net* h, const float* x, int N, int H, int W, int keep_all) {
  if (!h || !x || N <= 0 || H <= 0 || W <= 0) return fail(OCR_ERR_ARG, "bad argument");
  CAPI_HIP(rt_set_device(h->device));
  const size_t n = (size_t)N * H * W * 3;
  if (n > h->x_cap) {
    if (h->x_dev) (void)g_free(h->x_dev);
    h->x_dev = nullptr;
    h->x_cap = 0;
    CAPI_HIP(g_malloc(&h->x_dev, n * sizeof(float)));
    h->x_cap = n;
  }
  CAPI_HIP(hipMemcpyAsync(h->x_dev, x, n * sizeof(float), hipMemcpyHostToDevice, h->stream));
  h->net.set_keep_all(keep_all != 0);
  std::string err;
  if (!h->net.run(h->x_dev, N, H, W, h->stream, err)) return fail(h->net.refused() ? OCR_ERR_ARG : OCR_ERR_DEVICE, err);  // (a strict set_config's refusal)
  CAPI_HIP(g_stream_sync(h->stream));
  h->net.collect_timings();
  return OCR_OK;
}
/* the same network run again on the input already uploaded (timing loops) */
int ocr_srv_net_rerun(ocr_srv_net* h, int N, int H, int W, int iters) {
  if (!h || !h->x_dev || (size_t)N * H * W * 3 > h->x_cap) return fail(OCR_ERR_ARG, "no input resident");
  CAPI_HIP(rt_set_device(h->device));
  std::string err;
  for (int i = 0; i < iters; ++i)
    if (!h->net.run(h->x_dev, N, H, W, h->stream, err)) return fail(OCR_ERR_DEVICE, err);
  CAPI_HIP(g_stream_sync(h->stream));
  h->net.collect_timings();
  return OCR_OK;
}

int ocr_srv_net_num_tensors(ocr_srv_net* h) { return h ? h->net.ntensors() : 0; }

int ocr_srv_net_fetch(ocr_srv_net* h, int tid, float* out, size_t cap_floats, int dims[4]) {
  if (!h || !out || !dims) return fail(OCR_ERR_ARG, "null argument");
  CAPI_HIP(rt_set_device(h->device));
  std::vector<float> host;
  std::string err;
  if (!h->net.fetch_logical(tid, host, dims, h->stream, err)) return fail(OCR_ERR_ARG, err);
  if (host.size() > cap_floats) return fail(OCR_ERR_CAPACITY, "output buffer too small");
  memcpy(out, host.data(), host.size() * sizeof(float));
  return OCR_OK;
}

int ocr_srv_net_num_launches(ocr_srv_net* h) { return h ? h->net.num_launches() : 0; }

int ocr_srv_net_launch_info(ocr_srv_net* h, int i, char* name, size_t name_cap, int* out_tid, int* in_tids, int in_cap, int* n_in) {
  if (!h || !name || !out_tid || !in_tids || !n_in || name_cap == 0) return fail(OCR_ERR_ARG, "null argument");
  std::string nm;
  std::vector<int> ins;
  if (!h->net.launch_info(i, nm, *out_tid, ins)) return fail(OCR_ERR_ARG, "no such launch (or no binding yet)");
  if (nm.size() >= name_cap || (int)ins.size() > in_cap) return fail(OCR_ERR_CAPACITY, "buffer too small");
  memcpy(name, nm.c_str(), nm.size() + 1);
  for (size_t k = 0; k < ins.size(); ++k) in_tids[k] = ins[k];
  *n_in = (int)ins.size();
  return OCR_OK;
}

int ocr_srv_net_run_launches(ocr_srv_net* h, int first, int count) {
  if (!h) return fail(OCR_ERR_ARG, "null handle");
  CAPI_HIP(rt_set_device(h->device));
  std::string err;
  if (!h->net.run_launches(first, count, h->stream, err)) return fail(OCR_ERR_ARG, err);
  CAPI_HIP(g_stream_sync(h->stream));
  return OCR_OK;
}

int ocr_srv_net_upload(ocr_srv_net* h, int tid, const float* data, size_t count) {
  if (!h || !data) return fail(OCR_ERR_ARG, "null argument");
  CAPI_HIP(rt_set_device(h->device));
  std::string err;
  if (!h->net.upload_logical(tid, data, count, h->stream, err)) return fail(OCR_ERR_ARG, err);
  return OCR_OK;
}

// test hooks for the CTC head (tests/test_gpu_rec_tail.py): the head's partial mode as RecStage switches it, and the tail launch
// RecStage issues behind the network - launch_ctc_reduce on the head's partials with the handle's own ctc_slots() / ctc_step(),
// or launch_argmax_softmax on its logits - for the rows of the current binding
int ocr_srv_net_set_ctc(ocr_srv_net* h, int on) {
  if (!h) return fail(OCR_ERR_ARG, "null handle");
  h->net.set_ctc_partials(on != 0);
  return OCR_OK;
}
int ocr_srv_net_ctc_tail(ocr_srv_net* h, int32_t* amax, float* pmax, long cap_rows, long* rows, int* slots, int* step) {
  if (!h || !amax || !pmax || !rows || !slots || !step) return fail(OCR_ERR_ARG, "null argument");
  if (h->net.num_launches() == 0) return fail(OCR_ERR_ARG, "no binding yet: run ocr_srv_net_forward first");
  CAPI_HIP(rt_set_device(h->device));
  const auto& ot = h->net.tensor(h->net.output_tid());
  const long n = (long)ot.n * ot.h * ot.w;
  *rows = n;
  *slots = h->net.ctc_partials() ? h->net.ctc_slots() : 0;
  *step = h->net.ctc_partials() ? h->net.ctc_step() : 0;
  if (n < 1 || n > cap_rows) return fail(OCR_ERR_CAPACITY, "output buffers too small");
  int* da = nullptr;
  float* dp = nullptr;
  CAPI_HIP(g_malloc(&da, (size_t)n * sizeof(int)));
  if (g_malloc(&dp, (size_t)n * sizeof(float)) != hipSuccess) { (void)g_free(da); return fail(OCR_ERR_DEVICE, "hipMalloc failed"); }
  const float* out = (const float*)h->net.tensor_ptr(h->net.output_tid());
  if (h->net.ctc_partials())
    srv::launch_ctc_reduce(out, n, h->net.ctc_slots(), h->net.ctc_step(), da, dp, h->stream);
  else
    srv::launch_argmax_softmax(out, n, ot.c, ot.cs, da, dp, h->net.half(), h->stream);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = g_stream_sync(h->stream);
  if (e == hipSuccess) e = g_memcpy(amax, da, (size_t)n * sizeof(int), hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = g_memcpy(pmax, dp, (size_t)n * sizeof(float), hipMemcpyDeviceToHost);
  (void)g_free(da); (void)g_free(dp);
  CAPI_HIP(e);
  return OCR_OK;
}

int ocr_srv_net_timing(ocr_srv_net* h, int enable) {
  if (!h) return fail(OCR_ERR_ARG, "null handle");
  h->net.enable_timing(enable != 0);
  h->net.reset_timings();
  return OCR_OK;
}

int ocr_srv_net_timing_report(ocr_srv_net* h, char* buf, size_t cap) {
  if (!h || !buf) return fail(OCR_ERR_ARG, "null argument");
  size_t off = 0;
  for (auto& kv : h->net.timings()) {
    int n = snprintf(buf + off, cap > off ? cap - off : 0, "%s %.6f %ld %.0f %.0f\n", kv.first.c_str(), kv.second.ms, kv.second.count,
                     kv.second.flops, kv.second.bytes);
    if (n < 0 || off + n >= cap) return fail(OCR_ERR_CAPACITY, "report buffer too small");
    off += n;
  }
  if (off < cap) buf[off] = 0;
  return OCR_OK;
}

}  // extern "C"
