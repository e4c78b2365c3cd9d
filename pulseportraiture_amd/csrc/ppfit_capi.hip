// ppfit_capi.hip -- the context of libppfit: create / destroy, stream,
// options, workspace limit, timing, the phase profile and the selftest.
#include "ppfit_host.hpp"

// Source hash of this build (pulseportraiture_amd/build.py compares it with
// today's sources before reusing a built library).
#ifndef PPF_SRC_HASH
#define PPF_SRC_HASH "unbuilt"
#endif
extern "C" __attribute__((visibility("default"), used)) const char ppf_build_tag[] =
    "PPF_SRC_HASH=" PPF_SRC_HASH;

extern "C" {

int ppf_version(void) { return PPF_VERSION; }

int ppf_ctx_create(int device, ppf_ctx** out) {
  if (!out) return PPF_ERR_INVALID;
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return PPF_ERR_DEVICE;
  if (device < 0 || device >= n) return PPF_ERR_INVALID;
  if (hipSetDevice(device) != hipSuccess) return PPF_ERR_DEVICE;
  ppf_ctx* c = new ppf_ctx();
  c->device = device;
  *out = c;
  return PPF_OK;
}

void ppf_ctx_destroy(ppf_ctx* ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  (void)hipStreamSynchronize(ctx->stream);
  for (auto& t : ctx->pending) { (void)hipEventDestroy(t.a); (void)hipEventDestroy(t.b); }
  for (auto e : ctx->pool) (void)hipEventDestroy(e);
  for (auto e : ctx->sync_events) (void)hipEventDestroy(e);
  if (ctx->stream2) {
    (void)hipStreamSynchronize(ctx->stream2);
    (void)hipStreamDestroy(ctx->stream2);
  }
  for (auto& p : ctx->tw) (void)hipFree(p.second);
  for (auto& p : ctx->vp) (void)hipFree(p.second);
  if (ctx->active_h) (void)hipHostFree(ctx->active_h);
  for (auto e : ctx->scat_ev) if (e) (void)hipEventDestroy(e);
  for (auto& b : ctx->buf) if (b.p) (void)hipFree(b.p);
  delete ctx;
}

const char* ppf_last_error(const ppf_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int ppf_set_stream(ppf_ctx* ctx, void* stream) {
  if (!ctx) return PPF_ERR_INVALID;
  ctx->stream = reinterpret_cast<hipStream_t>(stream);
  return PPF_OK;
}

int ppf_set_pipeline(ppf_ctx* ctx, int32_t pieces) {
  if (!ctx || pieces < 0 || pieces > 64) return PPF_ERR_INVALID;
  ctx->pipe = pieces;
  return PPF_OK;
}

int ppf_set_option(ppf_ctx* ctx, int32_t option, int32_t value) {
  if (!ctx) return PPF_ERR_INVALID;
  if (option < 0 || option >= PPF_NUM_OPTS)
    return fail(ctx, PPF_ERR_INVALID, "unknown option %d", option);
  if (option == PPF_OPT_SCAT_TAIL ? value < 0 : (value != 0 && value != 1))
    return fail(ctx, PPF_ERR_INVALID, "option %d: bad value %d", option, value);
  ctx->opt[option] = value;
  return PPF_OK;
}

int ppf_get_option(const ppf_ctx* ctx, int32_t option, int32_t* value) {
  if (!ctx || !value || option < 0 || option >= PPF_NUM_OPTS) return PPF_ERR_INVALID;
  *value = ctx->opt[option];
  return PPF_OK;
}

int ppf_synchronize(ppf_ctx* ctx) {
  if (!ctx) return PPF_ERR_INVALID;
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return PPF_OK;
}

int ppf_set_workspace_limit(ppf_ctx* ctx, int64_t bytes) {
  if (!ctx || bytes <= 0) return PPF_ERR_INVALID;
  ctx->ws_limit = bytes;
  return PPF_OK;
}

int ppf_get_workspace_limit(const ppf_ctx* ctx, int64_t* bytes) {
  if (!ctx || !bytes) return PPF_ERR_INVALID;
  *bytes = ctx->ws_limit;
  return PPF_OK;
}

int ppf_set_trace(ppf_ctx* ctx, double* buf, int32_t cap) {
  if (!ctx || cap < 0 || (cap > 0 && !buf)) return PPF_ERR_INVALID;
  ctx->trace = buf;
  ctx->trace_cap = cap;
  return PPF_OK;
}

int ppf_set_timing(ppf_ctx* ctx, int enable) {
  if (!ctx) return PPF_ERR_INVALID;
  ctx->timing = enable != 0;
  return PPF_OK;
}

int ppf_get_kernel_time(ppf_ctx* ctx, int kid, double* total_ms, int64_t* launches) {
  if (!ctx || kid < 0 || kid >= PPF_NUM_KERNELS) return PPF_ERR_INVALID;
  if (int r = resolve_timing(ctx)) return r;
  if (total_ms) *total_ms = ctx->ktime[kid];
  if (launches) *launches = ctx->klaunch[kid];
  return PPF_OK;
}

int ppf_reset_kernel_times(ppf_ctx* ctx) {
  if (!ctx) return PPF_ERR_INVALID;
  if (int r = resolve_timing(ctx)) return r;
  for (int i = 0; i < PPF_NUM_KERNELS; ++i) { ctx->ktime[i] = 0.0; ctx->klaunch[i] = 0; }
  for (double& v : ctx->gram_ms) v = 0.0;
  return PPF_OK;
}

int ppf_get_pca_gram_times(ppf_ctx* ctx, double* ms) {
  if (!ctx || !ms) return PPF_ERR_INVALID;
  for (int i = 0; i < 5; ++i) ms[i] = ctx->gram_ms[i];
  return PPF_OK;
}

int ppf_phase_profile(ppf_ctx* ctx, int32_t enable, uint64_t* out) {
  if (!ctx) return fail(ctx, PPF_ERR_INVALID, "null context");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const size_t bytes = PPF_PHASE_N * sizeof(uint64_t);
  if (!ctx->buf[kPtime].p) {
    if (int r = ensure(ctx, ctx->buf[kPtime], bytes)) return r;
    HIPCHK(ctx, hipMemsetAsync(ctx->buf[kPtime].p, 0, bytes, ctx->stream));
  }
  if (out) HIPCHK(ctx, hipMemcpyAsync(out, ctx->buf[kPtime].p, bytes, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipMemsetAsync(ctx->buf[kPtime].p, 0, bytes, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  ctx->phase_prof = enable != 0;
  return PPF_OK;
}

int ppf_selftest(ppf_ctx* ctx, int32_t* fails) {
  if (!ctx || !fails) return fail(ctx, PPF_ERR_INVALID, "null argument");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  int* d = nullptr;
  HIPCHK(ctx, hipMalloc(&d, PPF_SELFTEST_N * sizeof(int)));
  (void)hipMemsetAsync(d, 0, PPF_SELFTEST_N * sizeof(int), ctx->stream);
  hipLaunchKernelGGL(k_selftest, dim3(1), dim3(64), 0, ctx->stream, d);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess)
    e = hipMemcpyAsync(fails, d, PPF_SELFTEST_N * sizeof(int), hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  (void)hipFree(d);
  if (e != hipSuccess) return fail(ctx, PPF_ERR_DEVICE, "selftest: %s", hipGetErrorString(e));
  return PPF_OK;
}

}  // extern "C"
