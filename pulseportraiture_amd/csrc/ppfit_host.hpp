// ppfit_host.hpp -- what the host files of libppfit (ppfit_capi*.hip, which
// implement include/ppfit.h) share: the context and its buffers, errors,
// tables, the event brackets, the kernel dispatch switches and the helpers of
// more than one family of entry points.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "ppfit.h"
#include "ppfit_kernels.hpp"
#include "ppfit_wsplan.hpp"

using namespace ppf;

namespace {

struct TimedLaunch {
  int kid;
  hipEvent_t a, b;
};

struct Buffer {
  void* p = nullptr;
  size_t bytes = 0;
};

// the device buffers of a context (ppf_ctx::buf), each grown on demand (ensure)
enum BufferId {
  kWs,     // per-chunk fit workspace
  kMspec,  // template spectra
  kAux,    // misc (synth templates, partial sums)
  kMmean,  // mean template spectra (guess)
  kPtime,  // k_fit_taylor phase clocks (ppf_phase_profile)
  kSpart,  // split scattering solve: block partials + running count
  kTmpl,   // template builders: knots / coefficients, rows and spectra
  kPack,   // pack status word, then ppf_fake_subints' fp64 rows (generic nbin)
  kNumBuffers
};

using TableCache = std::vector<std::pair<int, double2*>>;  // (nbin, table)
constexpr size_t kUnknown = ~(size_t)0;

}  // namespace

struct ppf_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  std::string err;
  int64_t ws_limit = (int64_t)32 << 30;
  // rfft twiddles and moment power tables (k_vpow), one per nbin (table_for)
  TableCache tw, vp;
  Buffer buf[kNumBuffers];
  // static LDS of k_fit_taylor on this context's device (taylor_lds_moments)
  size_t taylor_static_lds = kUnknown;
  int* active_h = nullptr;  // pinned host copies of the running count (two in flight)
  hipEvent_t scat_ev[2] = {nullptr, nullptr};  // their copies' completion
  hipStream_t stream2 = nullptr;        // second queue of the piece pipeline
  int pipe = 0;                         // pieces per chunk (0: default)
  std::vector<hipEvent_t> sync_events;  // ordering events (no timing)
  bool phase_prof = false;
  bool timing = false;
  std::vector<TimedLaunch> pending;
  std::vector<hipEvent_t> pool;
  double* trace = nullptr;  // solver trace buffer (ppf_set_trace), device
  int trace_cap = 0;
  // launch-schedule options (ppf_set_option; include/ppfit.h)
  int opt[PPF_NUM_OPTS] = {1, 1, 512, 1, 1, 0, 1, 1};
  double ktime[PPF_NUM_KERNELS] = {0};
  int64_t klaunch[PPF_NUM_KERNELS] = {0};
  // ppf_pca_gram_portraits under timing: mean pass, Gram tiles, slab sum, Jacobi, emit
  double gram_ms[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
};

namespace {

int fail(ppf_ctx* ctx, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  if (ctx) ctx->err = buf;
  return code;
}

#define HIPCHK(ctx, expr)                                                              \
  do {                                                                                 \
    hipError_t e_ = (expr);                                                            \
    if (e_ != hipSuccess)                                                              \
      return fail(ctx, PPF_ERR_DEVICE, "%s failed: %s", #expr, hipGetErrorString(e_)); \
  } while (0)

int ilog2_exact(int v) {
  if (v <= 0 || (v & (v - 1))) return -1;
  int l = 0;
  while ((1 << l) < v) ++l;
  return l;
}

// Any nbin in [16, 8192]: *logN = log2(nbin / 2) selects the FFT kernels of
// a power of two from 64 up (RowPow2<logN>); every other length gets a
// negative value that names its row transform -- kLogNSmooth the mixed-radix
// FFT (RowSmooth), kLogNDirect the direct sums (RowAny) -- by the one
// predicate row_kind (ppfit_smoothfft.hpp) under the context's option
// row_fft (no context: the default).  Only ROW_SWITCH and the fit's data pass
// tell the two apart; to every other site logN < 0 means "not a power of
// two", whichever it is.
constexpr int kLogNDirect = -1, kLogNSmooth = -2;
int check_nbin_any(ppf_ctx* ctx, int nbin, int* logN) {
  if (nbin < 16 || nbin > 8192)
    return fail(ctx, PPF_ERR_UNSUPPORTED, "nbin=%d: outside [16, 8192]", nbin);
  switch (row_kind(nbin, ctx ? ctx->opt[PPF_OPT_ROW_FFT] != 0 : true)) {
    case kRowPow2: *logN = ilog2_exact(nbin) - 1; break;
    case kRowSmooth: *logN = kLogNSmooth; break;
    default: *logN = kLogNDirect; break;
  }
  return PPF_OK;
}

// the table of nbin in a cache (n cells, created by make on first use)
template <typename F>
int table_for(ppf_ctx* ctx, TableCache& cache, int nbin, size_t n, F&& make,
              const double2** out) {
  for (auto& p : cache)
    if (p.first == nbin) { *out = p.second; return PPF_OK; }
  double2* t = nullptr;
  HIPCHK(ctx, hipMalloc(&t, n * sizeof(double2)));
  make(t);
  if (hipGetLastError() != hipSuccess) {  // not cached: the next call builds it again
    (void)hipFree(t);
    return fail(ctx, PPF_ERR_DEVICE, "table launch for nbin=%d failed", nbin);
  }
  cache.push_back({nbin, t});
  *out = t;
  return PPF_OK;
}

// rows of 16 cells (256 B): measured faster than 8 or 32
int nharm_pad(int nbin) { return ((nbin / 2 + 1) + 15) & ~15; }

// get_noise_PS: kc = int((1 - 1/4) * nharm) (pplib.py:2245)
int noise_kc(int nbin) { return (int)(0.75 * (double)(nbin / 2 + 1)); }

int ensure(ppf_ctx* ctx, Buffer& b, size_t bytes) {
  if (b.bytes >= bytes) return PPF_OK;
  if (b.p) {
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    HIPCHK(ctx, hipFree(b.p));
    b.p = nullptr;
    b.bytes = 0;
  }
  if (hipMalloc(&b.p, bytes) != hipSuccess)
    return fail(ctx, PPF_ERR_NOMEM, "hipMalloc(%zu) failed", bytes);
  b.bytes = bytes;
  return PPF_OK;
}

// a laid-out plan's arrays in the context's workspace buffer
int hold_workspace(ppf_ctx* ctx, WsPlan& ws) {
  if (int r = ensure(ctx, ctx->buf[kWs], ws.total)) return r;
  ws.base = static_cast<char*>(ctx->buf[kWs].p);
  return PPF_OK;
}

int twiddles(ppf_ctx* ctx, int nbin, const double2** out) {
  return table_for(ctx, ctx->tw, nbin, (size_t)nbin, [&](double2* t) {
    hipLaunchKernelGGL(k_twiddles, dim3((nbin + 255) / 256), dim3(256), 0, ctx->stream, t, nbin);
  }, out);
}

int vpow_table(ppf_ctx* ctx, int nbin, const double2** out) {
  const int rows = kVpowRows(nbin / 2);
  return table_for(ctx, ctx->vp, nbin, (size_t)rows * 16, [&](double2* t) {
    hipLaunchKernelGGL(k_vpow, dim3((rows * 16 + 255) / 256), dim3(256), 0, ctx->stream, t,
                       nbin, rows);
  }, out);
}

hipEvent_t ev_get(ppf_ctx* ctx) {
  if (!ctx->pool.empty()) {
    hipEvent_t e = ctx->pool.back();
    ctx->pool.pop_back();
    return e;
  }
  hipEvent_t e;
  (void)hipEventCreate(&e);
  return e;
}

// Launch helper: optional HIP-event bracket on the context stream.
template <typename F>
int timed_on(ppf_ctx* ctx, int kid, hipStream_t st, F&& launch) {
  hipEvent_t a = nullptr, b = nullptr;
  if (ctx->timing) {
    a = ev_get(ctx);
    b = ev_get(ctx);
    HIPCHK(ctx, hipEventRecord(a, st));
  }
  launch();
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(ctx, PPF_ERR_DEVICE, "kernel %d launch: %s", kid, hipGetErrorString(e));
  if (ctx->timing) {
    HIPCHK(ctx, hipEventRecord(b, st));
    ctx->pending.push_back({kid, a, b});
  }
  return PPF_OK;
}

template <typename F>
int timed(ppf_ctx* ctx, int kid, F&& launch) {
  return timed_on(ctx, kid, ctx->stream, launch);
}

int resolve_timing(ppf_ctx* ctx) {
  for (auto& t : ctx->pending) {
    HIPCHK(ctx, hipEventSynchronize(t.b));
    float ms = 0.f;
    HIPCHK(ctx, hipEventElapsedTime(&ms, t.a, t.b));
    ctx->ktime[t.kid] += (double)ms;
    ctx->klaunch[t.kid] += 1;
    ctx->pool.push_back(t.a);
    ctx->pool.push_back(t.b);
  }
  ctx->pending.clear();
  return PPF_OK;
}

// n elements of a device array on the host, once the context stream has
// brought them
template <typename T>
int fetch(ppf_ctx* ctx, const T* dev, size_t n, std::vector<T>& host) {
  host.resize(n);
  HIPCHK(ctx, hipMemcpyAsync(host.data(), dev, n * sizeof(T), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return PPF_OK;
}

// The host's look at n items' solver states (host: the caller's copy, reused
// from look to look): *all_done when every one has set `done`.
template <typename S>
int poll_done(ppf_ctx* ctx, const S* state, int n, std::vector<S>& host, bool* all_done) {
  if (int r = fetch(ctx, state, (size_t)n, host)) return r;
  *all_done = std::all_of(host.begin(), host.end(), [](const S& s) { return s.done != 0; });
  return PPF_OK;
}

// The row entry points' dispatch (check_nbin_any) and twiddles.
struct RowPlan {
  int logN;
  const double2* tw;
};

// the device step of a row entry point, after its argument checks
int row_device(ppf_ctx* ctx, int nbin, RowPlan* rp) {
  HIPCHK(ctx, hipSetDevice(ctx->device));
  return twiddles(ctx, nbin, &rp->tw);
}

// LG = log2(nbin / 2) of the FFT kernels' lengths
#define LOGN_CASES(...)                                      \
    case 5: { constexpr int LG = 5; __VA_ARGS__; } break;    \
    case 6: { constexpr int LG = 6; __VA_ARGS__; } break;    \
    case 7: { constexpr int LG = 7; __VA_ARGS__; } break;    \
    case 8: { constexpr int LG = 8; __VA_ARGS__; } break;    \
    case 9: { constexpr int LG = 9; __VA_ARGS__; } break;    \
    case 10: { constexpr int LG = 10; __VA_ARGS__; } break;  \
    case 11: { constexpr int LG = 11; __VA_ARGS__; } break;  \
    case 12: { constexpr int LG = 12; __VA_ARGS__; } break;

#define LOGN_SWITCH(L, ...)   \
  switch (L) {                \
    LOGN_CASES(__VA_ARGS__)   \
    default: break;           \
  }

// SWT_SWITCH: LOGN_SWITCH with LG = 0 for any other nbin (the generic-length sums)
#define SWT_SWITCH(L, ...)                                  \
  switch (L) {                                              \
    LOGN_CASES(__VA_ARGS__)                                 \
    default: { constexpr int LG = 0; __VA_ARGS__; } break;  \
  }

// The row kernels (ppfit_rowfft.hpp): the body sees the policy as Row, the
// kernel's last argument `row`, and lds(U), the dynamic LDS of a kernel that
// declares Row::Lds<U>.  L is check_nbin_any's logN.
#define ROW_ARM(ROW, INIT, NBIN, ...)                                        \
  {                                                                          \
    using Row = ROW;                                                         \
    const Row row INIT;                                                      \
    auto lds = [&](RowLds u) { return Row::lds(NBIN, u); };                  \
    __VA_ARGS__;                                                             \
  }
// the RowSmooth size class of NBIN
#define SMOOTH_SWITCH(NBIN, ...)                                             \
  do {                                                                       \
    SmoothPlan plan_;                                                        \
    smooth_plan(NBIN, &plan_);                                               \
    if (smooth_class(plan_.n) == 1024)                                       \
      ROW_ARM(RowSmooth<1024>, {plan_}, NBIN, __VA_ARGS__)                   \
    else                                                                     \
      ROW_ARM(RowSmooth<4096>, {plan_}, NBIN, __VA_ARGS__)                   \
  } while (0)
#define ROW_SWITCH(L, NBIN, ...)                                             \
  do {                                                                       \
    if ((L) == kLogNSmooth) {                                                \
      SMOOTH_SWITCH(NBIN, __VA_ARGS__);                                      \
    } else if ((L) < 0) {                                                    \
      ROW_ARM(RowAny, {NBIN}, NBIN, __VA_ARGS__)                             \
    } else {                                                                 \
      LOGN_SWITCH(L, ROW_ARM(RowPow2<LG>, {}, NBIN, __VA_ARGS__))            \
    }                                                                        \
  } while (0)

// WD: the instantiation with the per-channel tables in HBM (chan_tables)
#define WIDE_SWITCH(W, ...)                                \
  do {                                                     \
    if (W) { constexpr bool WD = true; __VA_ARGS__; }      \
    else { constexpr bool WD = false; __VA_ARGS__; }       \
  } while (0)

// JN: the instantiation of a Gaussian-fit kernel with join parameters
#define JOIN_SWITCH(J, ...)                                \
  do {                                                     \
    if (J) { constexpr bool JN = true; __VA_ARGS__; }      \
    else { constexpr bool JN = false; __VA_ARGS__; }       \
  } while (0)

// Template spectra for nrow rows of nbin (DC zeroed when zero_dc).
int model_spectra(ppf_ctx* ctx, int nrow, int nbin, const double* model, int zero_dc, Buffer& buf,
                  double2** M, double** pn, double** M2 = nullptr) {
  int logN;
  if (int r = check_nbin_any(ctx, nbin, &logN)) return r;
  const int NHP = nharm_pad(nbin);
  const size_t mbytes = (size_t)nrow * NHP * sizeof(double2);
  const size_t pbytes = ((size_t)nrow * sizeof(double) + 255) & ~(size_t)255;
  const size_t m2bytes = M2 ? (size_t)nrow * NHP * sizeof(double) : 0;
  if (int r = ensure(ctx, buf, mbytes + pbytes + m2bytes)) return r;
  *M = reinterpret_cast<double2*>(buf.p);
  *pn = reinterpret_cast<double*>(static_cast<char*>(buf.p) + mbytes);
  double* m2p = nullptr;
  if (M2) *M2 = m2p = reinterpret_cast<double*>(static_cast<char*>(buf.p) + mbytes + pbytes);
  const double2* tw;
  if (int r = twiddles(ctx, nbin, &tw)) return r;
  double2* Mp = *M;
  double* pp = *pn;
  return timed(ctx, PPF_K_MODEL_FFT, [&] {
    ROW_SWITCH(logN, nbin, hipLaunchKernelGGL(k_model_spec<Row>, dim3(nrow), dim3(kBlock),
                                              lds(kLdsRow), ctx->stream, model, Mp, pp, NHP,
                                              zero_dc, tw, m2p, row));
  });
}

// dynamic LDS of the Meta kernels' per-channel tables
size_t meta_lds(int nchan) { return align256((size_t)nchan * (5 * sizeof(double) + sizeof(int))); }

// ---------------------------------------------------------------------------
// Row transforms that several entry points dispatch, nrow rows on st.
// ---------------------------------------------------------------------------
void launch_rfft_rows(hipStream_t st, int logN, int nbin, int nrow, const double* in, double2* out,
                      const double2* tw) {
  ROW_SWITCH(logN, nbin, hipLaunchKernelGGL(k_rfft_rows<Row>, dim3(nrow), dim3(kBlock),
                                            lds(kLdsRow), st, in, out, tw, row));
}

void launch_irfft_rows(hipStream_t st, int logN, int nbin, int nrow, const double2* in,
                       double* out, const double2* tw) {
  ROW_SWITCH(logN, nbin, hipLaunchKernelGGL(k_irfft_rows<Row>, dim3(nrow), dim3(kBlock),
                                            lds(kLdsSpec), st, in, out, tw, row));
}

// rotation by phase and / or scattering by tau (either may be null)
void launch_rotate_rows(hipStream_t st, int logN, int nbin, int nrow, const double* in,
                        const double* phase, const double* tau, double* out, const double2* tw) {
  ROW_SWITCH(logN, nbin, hipLaunchKernelGGL(k_rotate_rows<Row>, dim3(nrow), dim3(kBlock),
                                            lds(kLdsRowInv), st, in, phase, tau, out, tw, row));
}

}  // namespace
