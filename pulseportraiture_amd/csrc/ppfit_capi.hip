// ppfit_capi.hip -- host side of libppfit: context, workspace, launches.
// Implements include/ppfit.h.
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

// Source hash of this build (pulseportraiture_amd/build.py compares it with
// today's sources before reusing a built library).
#ifndef PPF_SRC_HASH
#define PPF_SRC_HASH "unbuilt"
#endif
extern "C" __attribute__((visibility("default"), used)) const char ppf_build_tag[] =
    "PPF_SRC_HASH=" PPF_SRC_HASH;

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
  int opt[PPF_NUM_OPTS] = {1, 1, 512, 1, 1, 0, 1};
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
// a power of two from 64 up (RowPow2<logN>), -1 the direct sums (RowAny) for
// every other length.
int check_nbin_any(ppf_ctx* ctx, int nbin, int* logN) {
  if (nbin < 16 || nbin > 8192)
    return fail(ctx, PPF_ERR_UNSUPPORTED, "nbin=%d: outside [16, 8192]", nbin);
  const int l = ilog2_exact(nbin);
  *logN = l < 6 ? -1 : l - 1;
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

int twiddles(ppf_ctx* ctx, int nbin, const double2** out) {
  return table_for(ctx, ctx->tw, nbin, (size_t)nbin, [&](double2* t) {
    hipLaunchKernelGGL(k_twiddles, dim3((nbin + 255) / 256), dim3(256), 0, ctx->stream, t, nbin);
  }, out);
}

// Moments per channel of T slot 0 that k_fit_taylor's LDS copy holds:
// kTaylorBlocksPerCU blocks of (static LDS + Meta + nchan * tnl doubles) in a
// CU's LDS, whole KB per block.
int taylor_lds_moments(ppf_ctx* ctx, int nchan, size_t lds_meta) {
  if (ctx->taylor_static_lds == kUnknown) {
    size_t mx = 0;
    const void* ks[4] = {reinterpret_cast<const void*>(&k_fit_taylor<true, false>),
                         reinterpret_cast<const void*>(&k_fit_taylor<false, false>),
                         reinterpret_cast<const void*>(&k_fit_taylor<true, true>),
                         reinterpret_cast<const void*>(&k_fit_taylor<false, true>)};
    for (const void* k : ks) {
      hipFuncAttributes at;
      if (hipFuncGetAttributes(&at, k) != hipSuccess) return 0;
      mx = std::max(mx, at.sharedSizeBytes);
    }
    ctx->taylor_static_lds = mx;
  }
  const size_t stat = ctx->taylor_static_lds;
  const size_t per_block = (kLdsPerCU / kTaylorBlocksPerCU) & ~(size_t)1023;
  if (per_block <= stat + lds_meta) return 0;
  const size_t nl = (per_block - stat - lds_meta) / ((size_t)nchan * sizeof(double));
  return (int)std::min<size_t>(nl, kMT);
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

// i-th ordering event of the context (created on first use)
int sync_event(ppf_ctx* ctx, size_t i, hipEvent_t* out) {
  while (ctx->sync_events.size() <= i) {
    hipEvent_t e;
    HIPCHK(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    ctx->sync_events.push_back(e);
  }
  *out = ctx->sync_events[i];
  return PPF_OK;
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

#define LOGN_SWITCH(L, ...)                                  \
  switch (L) {                                               \
    case 5: { constexpr int LG = 5; __VA_ARGS__; } break;    \
    case 6: { constexpr int LG = 6; __VA_ARGS__; } break;    \
    case 7: { constexpr int LG = 7; __VA_ARGS__; } break;    \
    case 8: { constexpr int LG = 8; __VA_ARGS__; } break;    \
    case 9: { constexpr int LG = 9; __VA_ARGS__; } break;    \
    case 10: { constexpr int LG = 10; __VA_ARGS__; } break;  \
    case 11: { constexpr int LG = 11; __VA_ARGS__; } break;  \
    case 12: { constexpr int LG = 12; __VA_ARGS__; } break;  \
    default: break;                                          \
  }

// The row kernels (ppfit_rowfft.hpp): the body sees the policy as Row, the
// kernel's last argument `row`, and lds(U), the dynamic LDS of a kernel that
// declares Row::Lds<U>.
#define ROW_SWITCH(L, NBIN, ...)                                             \
  do {                                                                       \
    if ((L) < 0) {                                                           \
      using Row = RowAny;                                                    \
      const Row row{NBIN};                                                   \
      auto lds = [&](RowLds u) { return Row::lds(NBIN, u); };                \
      __VA_ARGS__;                                                           \
    } else {                                                                 \
      LOGN_SWITCH(L, using Row = RowPow2<LG>; const Row row{};               \
                  auto lds = [&](RowLds u) { return Row::lds(NBIN, u); };    \
                  __VA_ARGS__)                                               \
    }                                                                        \
  } while (0)

// WD: the instantiation with the per-channel tables in HBM (chan_tables)
#define WIDE_SWITCH(W, ...)                                \
  do {                                                     \
    if (W) { constexpr bool WD = true; __VA_ARGS__; }      \
    else { constexpr bool WD = false; __VA_ARGS__; }       \
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

size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

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

// ---------------------------------------------------------------------------
// ppf_fit_portrait_batch: workspace plan, stages, argument binding
// ---------------------------------------------------------------------------

// Workspace plan of one fit call: the arrays of a chunk of subints one after
// another in the context's workspace buffer.  Each array's per-subint size is
// written here and nowhere else.
struct FitWorkspace {
  struct Span { size_t off, per; };  // an array's offset and its bytes per subint
  Span X, R, sig, dsum, st, acc, wsc, T, G;
  int64_t chunk;         // subints per pass under the workspace limit
  size_t total;          // bytes of a chunk
  char* base = nullptr;  // the buffer, once it holds them

  FitWorkspace(int nchan, int NHP, bool taylor, bool wide, int64_t ws_limit, int64_t nsub) {
    const size_t bX = (size_t)nchan * NHP * sizeof(double2);
    const size_t bR = (size_t)NHP * sizeof(double2);
    const size_t bC = (size_t)nchan * sizeof(double);
    const size_t bAcc = (size_t)2 * nchan * 10 * sizeof(double);
    const size_t bW = (size_t)nchan * 8 * sizeof(double);
    const size_t bT = taylor ? (size_t)2 * nchan * kMT * sizeof(double) : 0;
    // per-channel tables in HBM (the WIDE kernels, ppfit_kernels.hpp chan_tables)
    const size_t bG = wide ? align256(std::max(meta_lds(nchan), xspec_dyn_lds(nchan))) : 0;
    // (2 bR: a second R-sized row that no kernel uses; it stays in the plan so
    // that a workspace limit gives the chunk, and so the launches, it always gave)
    const size_t per_sub = bX + bT + 2 * bR + 2 * bC + sizeof(SolveState) + bAcc + bW + bG;
    chunk = std::max<int64_t>(1, std::min<int64_t>(nsub, ws_limit / (int64_t)(per_sub + 1024)));
    total = 0;
    auto take = [&](size_t per) {
      const Span s{total, per};
      total = align256(total + (size_t)chunk * per);
      return s;
    };
    X = take(bX);
    R = take(bR);
    take(bR);
    sig = take(bC);
    dsum = take(bC);
    st = take(sizeof(SolveState));
    acc = take(bAcc);
    wsc = take(bW);
    T = take(bT);
    G = take(bG);
  }

  template <typename P>
  P* at(const Span& s, int sub) const {
    return reinterpret_cast<P*>(base + s.off + (size_t)sub * s.per);
  }

  // Every workspace pointer of the two argument structs, for the chunk's
  // subints sub ..: the whole chunk at sub = 0, a piece of it otherwise.
  void slice(int sub, SpecArgs& sa, FitArgs& fa) const {
    fa.X = sa.X = at<double2>(X, sub);
    fa.R = sa.R = at<double2>(R, sub);
    fa.sig = sa.sig = at<double>(sig, sub);
    fa.dsum = sa.dsum = at<double>(dsum, sub);
    fa.st = at<SolveState>(st, sub);
    fa.acc = at<double>(acc, sub);
    fa.wsc = at<double>(wsc, sub);
    fa.T = T.per ? at<double>(T, sub) : nullptr;
    fa.gdyn = sa.gdyn = G.per ? at<unsigned char>(G, sub) : nullptr;
    fa.gdyn_stride = sa.gdyn_stride = G.per;
  }
};

// What the stages of one fit call share: the data pass's dispatch and the
// kernels' dynamic LDS sizes.
struct FitLaunch {
  int logN, nbin;
  bool wide;
  size_t lds_meta;  // the Meta kernels (none for the WIDE ones)
  size_t lds_xspec, lds_guess, lds_taylor, lds_scat;
};

// The stages of a fit over n subints on st, each under its kernel id's event
// bracket.  Both schedules of ppf_fit_portrait_batch are made of these.

// The data pass.  Generic length: every row's rfft on the matrix cores into
// the X rows, then the per-subint pass (ppfit_generic.hip) (data-spectrum
// cache: the spectra into the cache's rows under STORE; under USE they are
// there already).
int stage_data(ppf_ctx* ctx, hipStream_t st, int n, const SpecArgs& sa, const FitLaunch& L) {
  const int nbin = L.nbin;
  return timed_on(ctx, PPF_K_DATA_XSPEC, st, [&] {
    if (L.logN < 0) {
      const int nrows = n * sa.nchan, NH = nbin / 2 + 1;
      const double* rows = sa.data + (size_t)sa.sub0 * sa.nchan * nbin;
      const dim3 g((nrows + kGenRows - 1) / kGenRows, (NH + 255) / 256);
      double2* dst = sa.D ? sa.D : sa.X;
      if (sa.spec_mode != PPF_SPEC_USE) {
        if (nbin <= kGenLdsTw)
          hipLaunchKernelGGL(k_dft_rows_mfma<true>, g, dim3(kBlock), dft_mfma_lds(nbin, true), st,
                             rows, dst, nrows, nbin, sa.NHP, sa.tw);
        else
          hipLaunchKernelGGL(k_dft_rows_mfma<false>, g, dim3(kBlock), dft_mfma_lds(nbin, false),
                             st, rows, dst, nrows, nbin, sa.NHP, sa.tw);
      }
      hipLaunchKernelGGL(k_data_post_gen, dim3(n), dim3(kBlock), 0, st, sa, nbin);
    }
    LOGN_SWITCH(L.logN, WIDE_SWITCH(L.wide, hipLaunchKernelGGL((k_data_xspec<LG, WD>), dim3(n),
                                                               dim3(XspecCfg<LG>::WPB * 64),
                                                               L.lds_xspec, st, sa)));
  });
}

int stage_guess(ppf_ctx* ctx, hipStream_t st, int n, const FitArgs& fa, const FitLaunch& L) {
  return timed_on(ctx, PPF_K_GUESS, st, [&] {
    if (fa.guess && fa.guess_wave) hipLaunchKernelGGL(k_guess_w, dim3(n), dim3(64), 0, st, fa);
    hipLaunchKernelGGL(k_guess, dim3(n), dim3(kBlock), fa.guess ? L.lds_guess : 0, st, fa);
  });
}

// the first moment pass as its own launch (PPF_OPT_FUSE_MOMENTS = 0; by
// default it runs inside k_fit_taylor); the moment passes form X from the
// data-spectrum cache when fa.Dsp is set
int stage_moments(ppf_ctx* ctx, hipStream_t st, int n, const FitArgs& fa) {
  if (ctx->opt[PPF_OPT_FUSE_MOMENTS]) return PPF_OK;
  return timed_on(ctx, PPF_K_MOMENTS, st, [&] {
    const dim3 g(n, (fa.nchan + 16 * kWaves - 1) / (16 * kWaves));
    if (fa.Dsp) hipLaunchKernelGGL((k_moments<4, true>), g, dim3(kBlock), 0, st, fa);
    else hipLaunchKernelGGL((k_moments<4, false>), g, dim3(kBlock), 0, st, fa);
  });
}

int stage_taylor(ppf_ctx* ctx, hipStream_t st, int n, const FitArgs& fa, const FitLaunch& L) {
  const bool mom = ctx->opt[PPF_OPT_FUSE_MOMENTS] != 0;
  const dim3 g(n), b(kBlock);
  const size_t lds = L.lds_taylor;
  return timed_on(ctx, PPF_K_FIT_TAYLOR, st, [&] {
    WIDE_SWITCH(L.wide, {
      if (fa.Dsp) {
        if (mom) hipLaunchKernelGGL((k_fit_taylor<true, true, WD>), g, b, lds, st, fa);
        else hipLaunchKernelGGL((k_fit_taylor<false, true, WD>), g, b, lds, st, fa);
      } else {
        if (mom) hipLaunchKernelGGL((k_fit_taylor<true, false, WD>), g, b, lds, st, fa);
        else hipLaunchKernelGGL((k_fit_taylor<false, false, WD>), g, b, lds, st, fa);
      }
    });
  });
}

// The post-fit, PPF_K_POST whichever kernels run.  post_wave_ok depends on
// launch-uniform values only, so exactly one of k_post_w and k_post<false> is
// launched: the other would return for every subint.  k_post<true> (tau != 0
// at the final point) is launched always: with tau not fitted that is the
// start value init[.][3], which lives in device memory, and reading it back
// would cost more than the empty launch.
int stage_post(ppf_ctx* ctx, hipStream_t st, int n, const FitArgs& fa, const FitLaunch& L) {
  return timed_on(ctx, PPF_K_POST, st, [&] {
    if (post_wave_ok(fa)) hipLaunchKernelGGL(k_post_w, dim3(n), dim3(64), L.lds_meta, st, fa);
    WIDE_SWITCH(L.wide, {
      if (!post_wave_ok(fa))
        hipLaunchKernelGGL((k_post<false, WD>), dim3(n), dim3(kBlock), L.lds_meta, st, fa);
      hipLaunchKernelGGL((k_post<true, WD>), dim3(n), dim3(kBlock), L.lds_meta, st, fa);
    });
  });
}

// errs_out: the sigma each channel was fitted with (the data pass's), for
// subints sa.sub0 .. of the batch
int stage_errs(ppf_ctx* ctx, hipStream_t st, int n, const SpecArgs& sa, double* errs_out) {
  if (!errs_out) return PPF_OK;
  HIPCHK(ctx, hipMemcpyAsync(errs_out + (size_t)sa.sub0 * sa.nchan, sa.sig,
                             (size_t)n * sa.nchan * sizeof(double), hipMemcpyDeviceToDevice, st));
  return PPF_OK;
}

// The trust-ncg scattering solve of nc subints with every evaluation split
// over blocks: k_solve<true> with each evaluation over `cur` blocks per subint
// (k_scat_sweep) and then every subint's solver step (k_scat_step).
int scat_split_solve(ppf_ctx* ctx, const FitArgs& fa, int nc, int split, size_t lds_scat) {
  const int nchan = fa.nchan;
  double* part = static_cast<double*>(ctx->buf[kSpart].p);
  int* ctrs = reinterpret_cast<int*>(part + (size_t)nc * ((nchan + 7) / 8) * kScatPart);
  HIPCHK(ctx, hipMemsetAsync(ctrs, 0, 2 * sizeof(int), ctx->stream));
  // iterations go in groups of kCheck launches; after each group its
  // running count is copied to pinned memory, and the host reads group
  // g's count only once group g + 1 is queued behind it, so the device
  // never waits for the host (a group launched after the last subint has
  // finished costs kCheck near-empty grids)
  constexpr int kCheck = 4;
  // once few subints are left (the tail of slow fits), each sweep is
  // spread over more blocks: one 8-channel group per wave.  The group
  // partials, and so every result, do not depend on the split.
  int cur = split;
  const int split_tail = std::max(split, std::min(32, (nchan + 31) / 32));
  // groups after the first are one hipGraph launch each (the same kernels
  // in the same order, captured once per call and split)
  hipGraphExec_t gx[2] = {nullptr, nullptr};
  auto graph_for = [&](int sp, hipGraphExec_t* ex) -> int {
    if (*ex) return PPF_OK;
    // captured on the context's second queue (the context stream may be
    // the legacy default stream, which cannot capture); launched on the
    // context stream
    if (!ctx->stream2)
      HIPCHK(ctx, hipStreamCreateWithFlags(&ctx->stream2, hipStreamNonBlocking));
    hipStream_t cs = ctx->stream2;
    hipGraph_t g = nullptr;
    HIPCHK(ctx, hipStreamBeginCapture(cs, hipStreamCaptureModeThreadLocal));
    for (int k = 0; k < kCheck; ++k) {
      hipLaunchKernelGGL(k_scat_sweep, dim3(nc, sp), dim3(kBlock), lds_scat, cs, fa, part, sp, 0);
      hipLaunchKernelGGL(k_scat_step, dim3(nc), dim3(64), 0, cs, fa, part, 0, ctrs, k & 1);
    }
    HIPCHK(ctx, hipStreamEndCapture(cs, &g));
    const hipError_t e = hipGraphInstantiate(ex, g, nullptr, nullptr, 0);
    (void)hipGraphDestroy(g);
    if (e != hipSuccess)
      return fail(ctx, PPF_ERR_DEVICE, "scattering solve graph: %s", hipGetErrorString(e));
    return PPF_OK;
  };
  // the execs are destroyed on every way out, error returns included, after
  // the work launched from them has drained
  struct GraphFree {
    hipGraphExec_t* g;
    hipStream_t st;
    ~GraphFree() {
      if (!g[0] && !g[1]) return;
      (void)hipStreamSynchronize(st);
      for (int i = 0; i < 2; ++i)
        if (g[i]) (void)hipGraphExecDestroy(g[i]);
    }
  } gfree{gx, ctx->stream};
  // group gi: iterations kCheck * gi ... + kCheck - 1 (the first is the
  // init sweep); its count lands in active_h[gi & 1]
  auto issue = [&](int gi) -> int {
    const int it0 = kCheck * gi;
    if (gi > 0 && ctx->opt[PPF_OPT_SCAT_GRAPH]) {
      hipGraphExec_t* ex = &gx[cur == split ? 0 : 1];
      if (int r = graph_for(cur, ex)) return r;
      if (int r = timed(ctx, PPF_K_SOLVE, [&] { (void)hipGraphLaunch(*ex, ctx->stream); }))
        return r;
    } else {
      for (int k = 0; k < kCheck; ++k) {
        const int init = it0 + k == 0 ? 1 : 0;
        if (int r = timed(ctx, PPF_K_SOLVE, [&] {
              hipLaunchKernelGGL(k_scat_sweep, dim3(nc, cur), dim3(kBlock), lds_scat, ctx->stream,
                                 fa, part, cur, init);
            }))
          return r;
        if (int r = timed(ctx, PPF_K_SOLVE, [&] {
              hipLaunchKernelGGL(k_scat_step, dim3(nc), dim3(64), 0, ctx->stream, fa, part, init,
                                 ctrs, (it0 + k) & 1);
            }))
          return r;
      }
    }
    HIPCHK(ctx, hipMemcpyAsync(ctx->active_h + (gi & 1), ctrs + ((it0 + kCheck - 1) & 1),
                               sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipEventRecord(ctx->scat_ev[gi & 1], ctx->stream));
    return PPF_OK;
  };
  // trust-ncg stops a fit at 1000 iterations (+ the init sweep)
  const int max_groups = (1001 + kCheck) / kCheck + 1;
  if (int r = issue(0)) return r;
  for (int gi = 0;; ++gi) {
    if (gi + 1 < max_groups)
      if (int r = issue(gi + 1)) return r;
    HIPCHK(ctx, hipEventSynchronize(ctx->scat_ev[gi & 1]));
    const int running = ctx->active_h[gi & 1];
    if (running == 0 || gi + 1 >= max_groups) break;
    if (running < ctx->opt[PPF_OPT_SCAT_TAIL]) cur = split_tail;
  }
  return PPF_OK;
}

bool fit_is_tnc(const ppf_fit_desc* d) {
  return d->method == PPF_METHOD_TNC || d->method == PPF_METHOD_TNC_LEGACY;
}
// X, the cross-spectrum, is written once by the data pass.  Phase-family
// subints are fitted from Taylor moments of it (k_fit_taylor); scattering
// fits, and every fit under PPF_SOLVE_EXACT, sweep it directly.
bool fit_is_exact(const ppf_fit_desc* d) { return (d->solver_flags & PPF_SOLVE_EXACT) != 0; }
bool fit_is_taylor(const ppf_fit_desc* d) {
  return !fit_is_exact(d) && d->method == PPF_METHOD_TRUST_NCG;
}

// The descriptor and result checks of ppf_fit_portrait_batch (nsub > 0);
// *logN as check_nbin_any gives it.
int check_fit_desc(ppf_ctx* ctx, const ppf_fit_desc* d, const ppf_fit_result* o, int* logN) {
  if (d->nchan <= 0 || d->nchan > PPF_MAX_NCHAN)
    return fail(ctx, PPF_ERR_UNSUPPORTED, "nchan=%d outside [1, %d]", d->nchan, PPF_MAX_NCHAN);
  if (d->nmodel <= 0) return fail(ctx, PPF_ERR_INVALID, "nmodel must be >= 1");
  if (d->method != PPF_METHOD_TRUST_NCG && !fit_is_tnc(d) && d->method != PPF_METHOD_NEWTON_CG)
    return fail(ctx, PPF_ERR_UNSUPPORTED, "Method %d is not implemented.", d->method);
  if (d->method == PPF_METHOD_TNC_LEGACY &&
      !(d->fit_flags[0] && d->fit_flags[1] && !d->fit_flags[2] && !d->fit_flags[3] &&
        !d->fit_flags[4]))
    return fail(ctx, PPF_ERR_INVALID, "legacy TNC fits phase and DM only (fit_flags [1,1,0,0,0])");
  if (d->solver_flags & ~(PPF_SOLVE_EXACT | PPF_SOLVE_EVAL | PPF_GUESS_DIRECT))
    return fail(ctx, PPF_ERR_INVALID, "unknown solver_flags bits 0x%x", d->solver_flags);
  if (!d->data || !d->model || !d->freqs || !d->P || !d->init || !d->nu_fit || !d->nu_out)
    return fail(ctx, PPF_ERR_INVALID, "missing required input pointer");
  if (!o->params || !o->param_errs || !o->nu_out || !o->cov || !o->scales || !o->scale_errs ||
      !o->channel_snrs || !o->chi2 || !o->red_chi2 || !o->snr || !o->nfev || !o->status)
    return fail(ctx, PPF_ERR_INVALID, "missing required output pointer");
  if (d->guess && d->guess_Ns < 2) return fail(ctx, PPF_ERR_INVALID, "guess_Ns must be >= 2");
  // nbin not a power of two: the generic-length data pass and template
  // spectra (ppfit_generic.hip); every solver kernel takes any nbin
  if (int r = check_nbin_any(ctx, d->nbin, logN)) return r;
  // data-spectrum cache: sig, dsum and R live in the caller's arrays, and
  // Taylor-path subints keep D instead of X (ppfit.h, PPF_SPEC_*)
  const int smode = d->spec_mode;
  if (smode != PPF_SPEC_NONE) {
    if (smode != PPF_SPEC_STORE && smode != PPF_SPEC_USE)
      return fail(ctx, PPF_ERR_INVALID, "spec_mode %d: PPF_SPEC_NONE, _STORE or _USE", smode);
    if (!d->spec || !d->spec_sig || !d->spec_dsum || !d->spec_R)
      return fail(ctx, PPF_ERR_INVALID, "spec_mode %d: spec, spec_sig, spec_dsum and spec_R "
                  "are required", smode);
    if (!fit_is_taylor(d) || d->fit_flags[3] || d->fit_flags[4])
      return fail(ctx, PPF_ERR_UNSUPPORTED, "the data-spectrum cache takes phase-family "
                  "trust-ncg fits only (tau and alpha not fitted, not PPF_SOLVE_EXACT)");
  }
  return PPF_OK;
}

// Everything of the two argument structs that comes from the descriptor, the
// result struct and the context's settings (templates and tables:
// fit_tables; workspace pointers: FitWorkspace::slice).
void bind_fit_args(const ppf_ctx* ctx, const ppf_fit_desc* d, const ppf_fit_result* o,
                   SpecArgs& sa, FitArgs& fa) {
  const int nbin = d->nbin;
  sa.nchan = fa.nchan = d->nchan;
  sa.NHP = fa.NHP = nharm_pad(nbin);
  sa.kc = fa.kc = noise_kc(nbin);
  sa.guess = fa.guess = d->guess;
  sa.data = d->data;
  sa.model_idx = fa.model_idx = d->model_idx;
  sa.freqs = fa.freqs = d->freqs;
  sa.errs = d->errs;
  sa.mask = fa.mask = d->chan_mask;
  sa.weights = d->weights;
  sa.P = fa.P = d->P;
  sa.init = fa.init = d->init;
  sa.guess_nu = fa.guess_nu = d->guess_nu;
  sa.log10_tau = fa.log10_tau = d->log10_tau;
  sa.fit_tau = d->fit_flags[3] ? 1 : 0;
  sa.exact = fit_is_exact(d) ? 1 : 0;
  sa.spec_mode = d->spec_mode;

  fa.nbin = nbin;
  fa.NH = nbin / 2 + 1;
  for (int i = 0; i < 5; ++i) fa.flags[i] = d->fit_flags[i] ? 1 : 0;
  fa.option = d->option;
  fa.is_toa = d->is_toa;
  fa.Ns = d->guess_Ns;
  fa.guess_wrap = d->guess_wrap;
  fa.solver_flags = d->solver_flags;
  fa.method = d->method;
  fa.guess_wave = ctx->opt[PPF_OPT_GUESS_WAVE];
  for (int i = 0; i < 5; ++i)
    for (int j = 0; j < 2; ++j) fa.bounds[i][j] = d->bounds ? d->bounds[2 * i + j] : NAN;
  fa.nu_fit = d->nu_fit;
  fa.nu_out = d->nu_out;
  fa.guess_tau = d->guess_tau;
  fa.ptime = ctx->phase_prof ? static_cast<unsigned long long*>(ctx->buf[kPtime].p) : nullptr;
  fa.trace = ctx->trace_cap > 0 ? ctx->trace : nullptr;
  fa.trace_cap = ctx->trace_cap;
  fa.o_params = o->params;
  fa.o_param_errs = o->param_errs;
  fa.o_nu_out = o->nu_out;
  fa.o_cov = o->cov;
  fa.o_scales = o->scales;
  fa.o_scale_errs = o->scale_errs;
  fa.o_channel_snrs = o->channel_snrs;
  fa.o_chi2 = o->chi2;
  fa.o_red_chi2 = o->red_chi2;
  fa.o_snr = o->snr;
  fa.o_nfev = o->nfev;
  fa.o_status = o->status;
  fa.o_init_used = o->init_used;
  fa.o_fun = o->fun;
  fa.o_cov_nosc = o->cov_nosc;
  fa.o_grad = o->grad;
  fa.o_hess = o->hess;
}

// Templates and tables of a fit call into the argument structs: twiddles,
// template spectra, the mean template spectrum for the unmasked guess and
// (Taylor path) the moment power table.
int fit_tables(ppf_ctx* ctx, const ppf_fit_desc* d, SpecArgs& sa, FitArgs& fa) {
  const int nchan = d->nchan, nbin = d->nbin, NHP = sa.NHP;
  if (int r = twiddles(ctx, nbin, &fa.tw)) return r;
  sa.tw = fa.tw;
  double2* M;
  double* pn;
  double* M2;
  if (int r = model_spectra(ctx, d->nmodel * nchan, nbin, d->model, 1, ctx->buf[kMspec], &M, &pn,
                            &M2))
    return r;
  sa.M = fa.M = M;
  fa.pn = pn;
  fa.M2 = M2;
  if (d->guess) {
    if (int r = ensure(ctx, ctx->buf[kMmean], (size_t)d->nmodel * NHP * sizeof(double2))) return r;
    double2* Mmean = reinterpret_cast<double2*>(ctx->buf[kMmean].p);
    fa.Mmean = Mmean;
    if (int r = timed(ctx, PPF_K_MODEL_FFT, [&] {
          hipLaunchKernelGGL(k_model_mean, dim3((NHP + 255) / 256, d->nmodel), dim3(256), 0,
                             ctx->stream, M, Mmean, nchan, NHP);
        }))
      return r;
  }
  if (fit_is_taylor(d))
    if (int r = vpow_table(ctx, nbin, &fa.vpow)) return r;
  return PPF_OK;
}

// ---------------------------------------------------------------------------
// ppf_pack_subints / ppf_fake_subints: the status word of the packing kernels
// ---------------------------------------------------------------------------
constexpr size_t kPackHead = 256;  // the status word's slice of buf[kPack]

// Zero the pack status word (buf[kPack] holds kPackHead + extra bytes).
int pack_begin(ppf_ctx* ctx, size_t extra, int** bad) {
  if (int r = ensure(ctx, ctx->buf[kPack], kPackHead + extra)) return r;
  *bad = static_cast<int*>(ctx->buf[kPack].p);
  HIPCHK(ctx, hipMemsetAsync(*bad, 0, sizeof(int), ctx->stream));
  return PPF_OK;
}

// Wait for the packing kernels and read the status word.
int pack_end(ppf_ctx* ctx, const int* bad) {
  int h = 0;
  HIPCHK(ctx, hipMemcpyAsync(&h, bad, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  if (h) return fail(ctx, PPF_ERR_INVALID, "non-finite sample: its row is stored as zeros");
  return PPF_OK;
}

int launch_pack(ppf_ctx* ctx, size_t rows, int nbin, const double* data, int16_t* raw, double* scl,
                double* offs, int* bad) {
  return timed(ctx, PPF_K_PACK, [&] {
    hipLaunchKernelGGL(k_pack, dim3((unsigned)rows), dim3(kBlock), 0, ctx->stream, data, nbin,
                       reinterpret_cast<short*>(raw), scl, offs, bad);
  });
}

}  // namespace

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

// ---------------------------------------------------------------------------
int ppf_fit_portrait_batch(ppf_ctx* ctx, const ppf_fit_desc* d, const ppf_fit_result* o) {
  if (!ctx || !d || !o) return fail(ctx, PPF_ERR_INVALID, "null argument");
  if (d->nsub <= 0) return PPF_OK;
  FitLaunch L;
  if (int r = check_fit_desc(ctx, d, o, &L.logN)) return r;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const int nchan = d->nchan, nbin = d->nbin, NH = nbin / 2 + 1;
  const bool tnc = fit_is_tnc(d), ncg = d->method == PPF_METHOD_NEWTON_CG;
  const bool exact = fit_is_exact(d), taylor = fit_is_taylor(d);
  SpecArgs sa{};
  FitArgs fa{};
  bind_fit_args(ctx, d, o, sa, fa);
  if (int r = fit_tables(ctx, d, sa, fa)) return r;

  // per-channel tables in HBM (the WIDE kernels, ppfit_kernels.hpp chan_tables)
  const bool wide = nchan > PPF_LDS_NCHAN || ctx->opt[PPF_OPT_HBM_TABLES] != 0;
  FitWorkspace ws(nchan, fa.NHP, taylor, wide, ctx->ws_limit, d->nsub);
  if (int r = ensure(ctx, ctx->buf[kWs], ws.total)) return r;
  ws.base = static_cast<char*>(ctx->buf[kWs].p);
  ws.slice(0, sa, fa);
  const int64_t chunk = ws.chunk;

  L.nbin = nbin;
  L.wide = wide;
  fa.post_wave = ctx->opt[PPF_OPT_POST_WAVE] && !wide;  // k_post_w reads its tables from LDS
  L.lds_meta = wide ? 0 : meta_lds(nchan);
  L.lds_xspec = wide ? 0 : xspec_dyn_lds(nchan);
  // k_fit_taylor keeps moments [0, tnl) of T slot 0 in LDS (all of them when
  // they fit beside kTaylorBlocksPerCU - 1 other blocks; none when WIDE)
  fa.tnl = taylor && !wide ? taylor_lds_moments(ctx, nchan, L.lds_meta) : 0;
  fa.tlds = fa.tnl > 0 ? (int)L.lds_meta : 0;
  L.lds_taylor = L.lds_meta + (size_t)nchan * fa.tnl * sizeof(double);
  L.lds_guess =
      (size_t)(fa.NHP + (d->guess ? pfa_scratch_slots(d->guess_Ns, NH) : 0)) * sizeof(double2);
  // trust-ncg scattering fits: every evaluation split over blocks of >= 64
  // fitted channels (k_scat_sweep / k_scat_step)
  // (PPF_OPT_SCAT_SPLIT = 0: one block per subint, k_solve<true>)
  const bool split_scat = ctx->opt[PPF_OPT_SCAT_SPLIT] && d->fit_flags[3] &&
                          d->method == PPF_METHOD_TRUST_NCG && !wide;
  const int split = std::max(1, std::min(16, nchan / 64));
  // the two-phase sweep's rows (any block's channel range at split or more)
  L.lds_scat = scat_sweep_lds(nchan, split);
  if (split_scat) {
    if (int r = ensure(ctx, ctx->buf[kSpart],
                       (size_t)chunk * ((nchan + 7) / 8) * kScatPart * sizeof(double) +
                           64 * sizeof(int) + 256))
      return r;
    if (!ctx->active_h) HIPCHK(ctx, hipHostMalloc(&ctx->active_h, 2 * sizeof(int)));
    for (auto& e : ctx->scat_ev)
      if (!e) HIPCHK(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming));
  }
  // the cache rows of subints sub .. (spec_mode set): D, and sig / dsum / R in
  // place of the workspace's
  auto bind_spec = [&](SpecArgs& sp, FitArgs& fp, int64_t sub) {
    if (d->spec_mode == PPF_SPEC_NONE) return;
    sp.D = reinterpret_cast<double2*>(d->spec) + (size_t)sub * nchan * fa.NHP;
    fp.Dsp = sp.D;
    sp.sig = d->spec_sig + (size_t)sub * nchan;
    fp.sig = sp.sig;
    sp.dsum = d->spec_dsum + (size_t)sub * nchan;
    fp.dsum = sp.dsum;
    sp.R = reinterpret_cast<double2*>(d->spec_R) + (size_t)sub * fa.NHP;
    fp.R = sp.R;
  };
  // Phase-family Taylor path, several pieces per chunk on two queues: piece
  // p's data pass starts when piece p-1's has finished, so the latency-bound
  // guess / fit / post-fit kernels of one piece run beside the HBM-bound
  // data pass of the next.  Each piece owns its slice of the workspace.
  const int pieces = ctx->pipe > 0 ? ctx->pipe : 1;
  const bool phase_family = !d->fit_flags[3] && !d->fit_flags[4];
  if (taylor && !tnc && phase_family && pieces > 1) {
    if (!ctx->stream2)
      HIPCHK(ctx, hipStreamCreateWithFlags(&ctx->stream2, hipStreamNonBlocking));
    hipEvent_t start, prev_x = nullptr;
    if (int r = sync_event(ctx, 0, &start)) return r;
    HIPCHK(ctx, hipEventRecord(start, ctx->stream));  // templates, tables, earlier calls
    HIPCHK(ctx, hipStreamWaitEvent(ctx->stream2, start, 0));
    size_t ev = 1;
    for (int64_t s0 = 0; s0 < d->nsub; s0 += chunk) {
      const int nc = (int)std::min<int64_t>(chunk, d->nsub - s0);
      const int np = std::min(pieces, nc);
      const int ps = (nc + np - 1) / np;
      for (int p = 0; p * ps < nc; ++p) {
        const int off = p * ps, n = std::min(ps, nc - off);
        hipStream_t st = (p & 1) ? ctx->stream2 : ctx->stream;
        SpecArgs sp = sa;
        FitArgs fp = fa;
        sp.sub0 = fp.sub0 = (int)s0 + off;
        ws.slice(off, sp, fp);
        bind_spec(sp, fp, s0 + off);
        if (prev_x) HIPCHK(ctx, hipStreamWaitEvent(st, prev_x, 0));
        if (int r = stage_data(ctx, st, n, sp, L)) return r;
        if (int r = sync_event(ctx, ev++, &prev_x)) return r;
        HIPCHK(ctx, hipEventRecord(prev_x, st));
        if (int r = stage_guess(ctx, st, n, fp, L)) return r;
        if (int r = stage_moments(ctx, st, n, fp)) return r;
        if (int r = stage_taylor(ctx, st, n, fp, L)) return r;
        // subints the Taylor path does not take (tau != 0 at the start, not
        // fitted): the one-workgroup scattering solve and post-fit, as on
        // one queue (both exit at once for every other subint)
        if (int r = timed_on(ctx, PPF_K_SOLVE, st, [&] {
              WIDE_SWITCH(wide, hipLaunchKernelGGL((k_solve<true, WD>), dim3(n), dim3(kBlock),
                                                   L.lds_meta, st, fp));
            }))
          return r;
        if (int r = stage_post(ctx, st, n, fp, L)) return r;
        if (int r = stage_errs(ctx, st, n, sp, o->errs_out)) return r;
      }
    }
    // join: the caller's stream sees every piece
    hipEvent_t done;
    if (int r = sync_event(ctx, ev++, &done)) return r;
    HIPCHK(ctx, hipEventRecord(done, ctx->stream2));
    HIPCHK(ctx, hipStreamWaitEvent(ctx->stream, done, 0));
    return PPF_OK;
  }
  // One queue, the whole chunk at a time.
  hipStream_t st = ctx->stream;
  for (int64_t s0 = 0; s0 < d->nsub; s0 += chunk) {
    const int nc = (int)std::min<int64_t>(chunk, d->nsub - s0);
    sa.sub0 = fa.sub0 = (int)s0;
    bind_spec(sa, fa, s0);
    if (int r = stage_data(ctx, st, nc, sa, L)) return r;
    if (int r = stage_guess(ctx, st, nc, fa, L)) return r;
    // each subint runs in exactly one of the exact phase-only / scattering /
    // fused Taylor variants (the others exit at once)
    if (int r = timed(ctx, PPF_K_SOLVE, [&] {
          const dim3 g(nc), b(kBlock);
          const size_t lds = L.lds_meta;
          WIDE_SWITCH(wide, {
            if (tnc) {
              hipLaunchKernelGGL((k_tnc<false, WD>), g, b, lds, st, fa);
              hipLaunchKernelGGL((k_tnc<true, WD>), g, b, lds, st, fa);
              return;
            }
            if (ncg) {
              hipLaunchKernelGGL((k_ncg<false, WD>), g, b, lds, st, fa);
              hipLaunchKernelGGL((k_ncg<true, WD>), g, b, lds, st, fa);
              return;
            }
            if (exact) hipLaunchKernelGGL((k_solve<false, WD>), g, b, lds, st, fa);
            if (!split_scat) hipLaunchKernelGGL((k_solve<true, WD>), g, b, lds, st, fa);
          });
        }))
      return r;
    if (split_scat && !tnc && !ncg)
      if (int r = scat_split_solve(ctx, fa, nc, split, L.lds_scat)) return r;
    if (taylor) {
      if (int r = stage_moments(ctx, st, nc, fa)) return r;
      if (int r = stage_taylor(ctx, st, nc, fa, L)) return r;
    }
    if (int r = stage_post(ctx, st, nc, fa, L)) return r;
    if (int r = stage_errs(ctx, st, nc, sa, o->errs_out)) return r;
  }
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

// Number of template rows = 1 + max(model_idx) (device array or null: one
// row); the caller sizes model.  A negative index is an error.
static int count_model_rows(ppf_ctx* ctx, const int32_t* model_idx, int32_t nprof, int* nmodel) {
  *nmodel = 1;
  if (!model_idx) return PPF_OK;
  std::vector<int32_t> h(nprof);
  HIPCHK(ctx, hipMemcpyAsync(h.data(), model_idx, nprof * sizeof(int32_t), hipMemcpyDeviceToHost,
                             ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  for (int32_t v : h) {
    if (v < 0) return fail(ctx, PPF_ERR_INVALID, "negative model_idx");
    *nmodel = std::max(*nmodel, (int)v + 1);
  }
  return PPF_OK;
}

int ppf_phase_shift_batch(ppf_ctx* ctx, int32_t nprof, int32_t nbin, const double* data,
                          const double* model, const int32_t* model_idx, const double* noise,
                          int32_t Ns, double lo, double hi, double* out) {
  if (!ctx || !data || !model || !out) return fail(ctx, PPF_ERR_INVALID, "null argument");
  if (nprof <= 0) return PPF_OK;
  if (Ns < 2) return fail(ctx, PPF_ERR_INVALID, "Ns must be >= 2");
  int logN;
  if (int r = check_nbin_any(ctx, nbin, &logN)) return r;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  int nmodel;
  if (int r = count_model_rows(ctx, model_idx, nprof, &nmodel)) return r;
  double2* M;
  double* pn;
  if (int r = model_spectra(ctx, nmodel, nbin, model, 1, ctx->buf[kAux], &M, &pn)) return r;
  const double2* tw;
  if (int r = twiddles(ctx, nbin, &tw)) return r;
  PhaseShiftArgs pa;
  pa.NHP = nharm_pad(nbin);
  pa.kc = noise_kc(nbin);
  pa.Ns = Ns;
  pa.lo = lo;
  pa.hi = hi;
  pa.data = data;
  pa.M = M;
  pa.model_idx = model_idx;
  pa.noise = noise;
  pa.out = out;
  pa.tw = tw;
  return timed(ctx, PPF_K_PHASE_SHIFT, [&] {
    ROW_SWITCH(logN, nbin, hipLaunchKernelGGL(k_phase_shift<Row>, dim3(nprof), dim3(kBlock),
                                              lds(kLdsRowSpec), ctx->stream, pa, row));
  });
}

int ppf_phase_tau_batch(ppf_ctx* ctx, int32_t nprof, int32_t nbin, const double* data,
                        const double* model, const int32_t* model_idx, const double* noise,
                        const double* tau0, int32_t log10_tau, double* out, int32_t* status,
                        int32_t* nfev) {
  if (!ctx || !data || !model || !out || !status || !nfev)
    return fail(ctx, PPF_ERR_INVALID, "null argument");
  if (nprof <= 0) return PPF_OK;
  int logN;
  if (int r = check_nbin_any(ctx, nbin, &logN)) return r;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  int nmodel;
  if (int r = count_model_rows(ctx, model_idx, nprof, &nmodel)) return r;
  const double2* tw;
  if (int r = twiddles(ctx, nbin, &tw)) return r;
  // the template rows' spectra once, then the profiles' in chunks of the
  // workspace limit, each followed by its fits
  const size_t NH = (size_t)nbin / 2 + 1, brow = NH * sizeof(double2);
  if (int r = ensure(ctx, ctx->buf[kAux], (size_t)nmodel * brow)) return r;
  double2* M = static_cast<double2*>(ctx->buf[kAux].p);
  if (int r = timed(ctx, PPF_K_MODEL_FFT, [&] {
        launch_rfft_rows(ctx->stream, logN, nbin, nmodel, model, M, tw);
      }))
    return r;
  const int64_t chunk =
      std::max<int64_t>(1, std::min<int64_t>(nprof, ctx->ws_limit / (int64_t)brow));
  if (int r = ensure(ctx, ctx->buf[kWs], (size_t)chunk * brow)) return r;
  double2* D = static_cast<double2*>(ctx->buf[kWs].p);
  NbScatArgs na;
  na.nbin = nbin;
  na.NH = (int)NH;
  na.kc = noise_kc(nbin);
  na.log10_tau = log10_tau != 0;
  na.D = D;
  na.M = M;
  const int nh = nbin / 2;  // harmonics 1 .. nh; 64 per register slot
  const int nj = nh <= 64 ? 1 : nh <= 128 ? 2 : nh <= 256 ? 4 : nh <= 512 ? 8 : nh <= 1024 ? 16 : 0;
  for (int64_t r0 = 0; r0 < nprof; r0 += chunk) {
    const int nc = (int)std::min<int64_t>(chunk, nprof - r0);
    if (int r = timed(ctx, PPF_K_DATA_XSPEC, [&] {
          launch_rfft_rows(ctx->stream, logN, nbin, nc, data + (size_t)r0 * nbin, D, tw);
        }))
      return r;
    na.nprof = nc;
    na.model_idx = model_idx ? model_idx + r0 : nullptr;
    na.noise = noise ? noise + r0 : nullptr;
    na.tau0 = tau0 ? tau0 + r0 : nullptr;
    na.out = out + (size_t)r0 * 9;
    na.status = status + r0;
    na.nfev = nfev + r0;
    const dim3 g((nc + kWaves - 1) / kWaves), b(kBlock);
    if (int r = timed(ctx, PPF_K_SOLVE, [&] {
          switch (nj) {
            case 1: hipLaunchKernelGGL(k_nbscat<1>, g, b, 0, ctx->stream, na); break;
            case 2: hipLaunchKernelGGL(k_nbscat<2>, g, b, 0, ctx->stream, na); break;
            case 4: hipLaunchKernelGGL(k_nbscat<4>, g, b, 0, ctx->stream, na); break;
            case 8: hipLaunchKernelGGL(k_nbscat<8>, g, b, 0, ctx->stream, na); break;
            case 16: hipLaunchKernelGGL(k_nbscat<16>, g, b, 0, ctx->stream, na); break;
            default: hipLaunchKernelGGL(k_nbscat<0>, g, b, 0, ctx->stream, na); break;
          }
        }))
      return r;
  }
  return PPF_OK;
}

int ppf_rotate_rows(ppf_ctx* ctx, int32_t nrow, int32_t nbin, const double* in,
                    const double* phase, double* out) {
  if (!ctx || !in || !phase || !out) return fail(ctx, PPF_ERR_INVALID, "null argument");
  if (nrow <= 0) return PPF_OK;
  int logN;
  if (int r = check_nbin_any(ctx, nbin, &logN)) return r;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const double2* tw;
  if (int r = twiddles(ctx, nbin, &tw)) return r;
  return timed(ctx, PPF_K_ROTATE, [&] {
    launch_rotate_rows(ctx->stream, logN, nbin, nrow, in, phase, nullptr, out, tw);
  });
}

int ppf_scatter_rotate_rows(ppf_ctx* ctx, int32_t nrow, int32_t nbin, const double* in,
                            const double* phase, const double* tau, double* out) {
  if (!ctx || !in || !out) return fail(ctx, PPF_ERR_INVALID, "null argument");
  if (nrow <= 0) return PPF_OK;
  int logN;
  if (int r = check_nbin_any(ctx, nbin, &logN)) return r;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const double2* tw;
  if (int r = twiddles(ctx, nbin, &tw)) return r;
  if (!phase) return fail(ctx, PPF_ERR_INVALID, "phase must be given (zeros for none)");
  return timed(ctx, PPF_K_ROTATE, [&] {
    launch_rotate_rows(ctx->stream, logN, nbin, nrow, in, phase, tau, out, tw);
  });
}

int ppf_spline_portraits(ppf_ctx* ctx, int32_t nrow, int32_t nbin_in, int32_t nbin, int32_t neig,
                         const double* mean_prof, const double* eigvec, int32_t nknot, int32_t k,
                         const double* t, const double* c, int32_t ncoef, const double* freqs,
                         double* out) {
  if (!ctx || !mean_prof || !freqs || !out || (neig > 0 && (!eigvec || !t || !c)))
    return fail(ctx, PPF_ERR_INVALID, "null argument");
  if (nrow <= 0) return PPF_OK;
  if (neig < 0 || neig > kMaxEig)
    return fail(ctx, PPF_ERR_UNSUPPORTED, "neig=%d: at most %d eigenvectors", neig, kMaxEig);
  if (neig > 0) {
    if (k < 1 || k > kMaxSplineK)
      return fail(ctx, PPF_ERR_UNSUPPORTED, "spline degree k=%d: 1..%d", k, kMaxSplineK);
    if (nknot < 2 * (k + 1) || ncoef < nknot - k - 1)
      return fail(ctx, PPF_ERR_INVALID, "nknot=%d, ncoef=%d: need nknot >= 2(k+1), ncoef >= nknot-k-1",
                  nknot, ncoef);
  }
  if (nbin_in <= 0) return fail(ctx, PPF_ERR_INVALID, "nbin_in=%d", nbin_in);
  int logI = 0, logO = 0;
  const bool resample = nbin_in != nbin;
  if (resample) {
    if (int r = check_nbin_any(ctx, nbin_in, &logI)) return r;
    if (int r = check_nbin_any(ctx, nbin, &logO)) return r;
  } else if (nbin <= 0) {
    return fail(ctx, PPF_ERR_INVALID, "nbin=%d", nbin);
  }
  HIPCHK(ctx, hipSetDevice(ctx->device));
  // device copies of the knots and coefficients, then (resampling) the rows
  // at nbin_in and both spectra
  const size_t ntc = neig > 0 ? (size_t)nknot + (size_t)neig * ncoef : 0;
  const size_t nrows_in = resample ? (size_t)nrow * nbin_in : 0;
  const size_t hin = (size_t)nbin_in / 2 + 1, hout = (size_t)nbin / 2 + 1;
  const size_t nspec = resample ? (size_t)nrow * (hin + hout) * 2 : 0;
  if (int r = ensure(ctx, ctx->buf[kTmpl], (ntc + nrows_in + nspec) * sizeof(double))) return r;
  double* base = static_cast<double*>(ctx->buf[kTmpl].p);
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));  // tmpl may still feed an earlier launch
  SplineArgs s;
  s.nbin = nbin_in;
  s.neig = neig;
  s.n = nknot;
  s.k = k;
  s.ncoef = ncoef;
  s.t = base;
  s.c = base + nknot;
  s.mean = mean_prof;
  s.eigvec = eigvec;
  if (neig > 0) {
    HIPCHK(ctx, hipMemcpy(base, t, (size_t)nknot * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(ctx, hipMemcpy(base + nknot, c, (size_t)neig * ncoef * sizeof(double),
                          hipMemcpyHostToDevice));
  }
  double* rows = resample ? base + ntc : out;
  if (int r = timed(ctx, PPF_K_MODEL_FFT, [&] {
        hipLaunchKernelGGL(k_spline_rows, dim3(nrow), dim3(256), 0, ctx->stream, s, freqs, rows);
      }))
    return r;
  if (!resample) return PPF_OK;
  double2* X = reinterpret_cast<double2*>(base + ntc + nrows_in);
  double2* Y = X + (size_t)nrow * hin;
  const double2 *twi, *two;
  if (int r = twiddles(ctx, nbin_in, &twi)) return r;
  if (int r = twiddles(ctx, nbin, &two)) return r;
  // ss.resample introduces a shift, undone by rotate_portrait (pplib.py:953-955)
  const double shift = 0.5 * (1.0 / (double)nbin - 1.0 / (double)nbin_in);
  const size_t ny = (size_t)nrow * hout;
  return timed(ctx, PPF_K_MODEL_FFT, [&] {
    launch_rfft_rows(ctx->stream, logI, nbin_in, nrow, rows, X, twi);
    hipLaunchKernelGGL(k_resample_spec, dim3((unsigned)((ny + 255) / 256)), dim3(256), 0,
                       ctx->stream, X, nbin_in, nbin, shift, nrow, Y);
    launch_irfft_rows(ctx->stream, logO, nbin, nrow, Y, out, two);
  });
}

int ppf_instrumental_response_rows(ppf_ctx* ctx, int32_t nrow, int32_t nbin, const double* in,
                                   int32_t nw, const double* wids, const int32_t* types,
                                   double DM, double chan_bw, double P, const double* freqs,
                                   double* out) {
  if (!ctx || !out || (nw > 0 && (!wids || !types)) || (DM != 0.0 && !freqs))
    return fail(ctx, PPF_ERR_INVALID, "null argument");
  if (nrow <= 0) return PPF_OK;
  if (nw < 0 || nw > kMaxIrf)
    return fail(ctx, PPF_ERR_UNSUPPORTED, "nw=%d: at most %d responses", nw, kMaxIrf);
  IrArgs g;
  g.nw = nw;
  g.fwhm = 2.0 * std::sqrt(2.0 * std::log(2.0));
  for (int w = 0; w < nw; ++w) {
    if (types[w] != 0 && types[w] != 1)
      return fail(ctx, PPF_ERR_INVALID, "irf type %d: 0 (rect) or 1 (gauss)", types[w]);
    if (!(wids[w] > 0.0))
      return fail(ctx, PPF_ERR_INVALID, "irf width %g: must be > 0", wids[w]);
    if (types[w] == 1) {
      // a = 1 / (2 sqrt 2 sigma_t) >= 6 keeps the dropped exp(-a^2) w(z) term below 2.4e-16
      const double st = wids[w] / g.fwhm;
      if (1.0 / (2.0 * M_SQRT2 * st) < 6.0)
        return fail(ctx, PPF_ERR_UNSUPPORTED,
                    "gauss irf FWHM %g rot: supported up to %.4f rot", wids[w],
                    g.fwhm / (12.0 * M_SQRT2));
    }
    g.type[w] = types[w];
    g.wid[w] = wids[w];
  }
  g.dm_wid_num = DM != 0.0 ? 8.3e-6 * chan_bw : 0.0;
  g.P = P;
  if (DM != 0.0 && !(P > 0.0)) return fail(ctx, PPF_ERR_INVALID, "P=%g", P);
  int logN;
  if (int r = check_nbin_any(ctx, nbin, &logN)) return r;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const size_t nh = (size_t)nbin / 2 + 1, n = (size_t)nrow * nh;
  const unsigned grid = (unsigned)((n + 255) / 256);
  if (!in)  // the response table R [nrow][nharm] itself
    return timed(ctx, PPF_K_MODEL_FFT, [&] {
      hipLaunchKernelGGL(k_ir_spec, dim3(grid), dim3(256), 0, ctx->stream, nullptr, out, nrow,
                         (int)nh, g, freqs);
    });
  if (int r = ensure(ctx, ctx->buf[kTmpl], n * sizeof(double2))) return r;
  double2* X = static_cast<double2*>(ctx->buf[kTmpl].p);
  const double2* tw;
  if (int r = twiddles(ctx, nbin, &tw)) return r;
  return timed(ctx, PPF_K_MODEL_FFT, [&] {
    launch_rfft_rows(ctx->stream, logN, nbin, nrow, in, X, tw);
    hipLaunchKernelGGL(k_ir_spec, dim3(grid), dim3(256), 0, ctx->stream, X, nullptr, nrow, (int)nh,
                       g, freqs);
    launch_irfft_rows(ctx->stream, logN, nbin, nrow, X, out, tw);
  });
}

int ppf_tscrunch(ppf_ctx* ctx, int32_t nsub, int32_t npol, int32_t nchan, int32_t nbin,
                 const double* data, const double* weights, double* out, double* wsum) {
  if (!ctx || !data || !weights || !out) return fail(ctx, PPF_ERR_INVALID, "null argument");
  if (nsub <= 0 || npol <= 0 || nchan <= 0 || nbin <= 0)
    return fail(ctx, PPF_ERR_INVALID, "empty archive (%d, %d, %d, %d)", nsub, npol, nchan, nbin);
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const size_t total = (size_t)npol * nchan * nbin;
  return timed(ctx, PPF_K_MODEL_FFT, [&] {
    hipLaunchKernelGGL(k_tscrunch, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream,
                       data, weights, nsub, npol, nchan, nbin, out, wsum);
  });
}

int ppf_irfft_rows(ppf_ctx* ctx, int32_t nrow, int32_t nbin, const double* spec, double* out) {
  if (!ctx || !spec || !out) return fail(ctx, PPF_ERR_INVALID, "null argument");
  if (nrow <= 0) return PPF_OK;
  int logN;
  if (int r = check_nbin_any(ctx, nbin, &logN)) return r;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const double2* tw;
  if (int r = twiddles(ctx, nbin, &tw)) return r;
  const double2* sp = reinterpret_cast<const double2*>(spec);
  return timed(ctx, PPF_K_IRFFT, [&] {
    launch_irfft_rows(ctx->stream, logN, nbin, nrow, sp, out, tw);
  });
}

int ppf_noise_rows_frac(ppf_ctx* ctx, int32_t nrow, int32_t nbin, double frac, const double* in,
                        double* out) {
  if (!ctx || !in || !out) return fail(ctx, PPF_ERR_INVALID, "null argument");
  if (nrow <= 0) return PPF_OK;
  int logN;
  if (int r = check_nbin_any(ctx, nbin, &logN)) return r;
  if (!(frac > 1.0) || !std::isfinite(frac))
    return fail(ctx, PPF_ERR_INVALID, "frac=%g: must be > 1 and finite", frac);
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const double2* tw;
  if (int r = twiddles(ctx, nbin, &tw)) return r;
  // pplib.py:2245, kc = int((1 - frac**-1) * len(pows)); frac = 4 is noise_kc
  const int kc = (int)((1.0 - 1.0 / frac) * (double)(nbin / 2 + 1));
  return timed(ctx, PPF_K_NOISE, [&] {
    ROW_SWITCH(logN, nbin, hipLaunchKernelGGL(k_noise_rows<Row>, dim3(nrow), dim3(kBlock),
                                              lds(kLdsRow), ctx->stream, in, out, kc, tw, row));
  });
}

int ppf_noise_rows(ppf_ctx* ctx, int32_t nrow, int32_t nbin, const double* in, double* out) {
  return ppf_noise_rows_frac(ctx, nrow, nbin, 4.0, in, out);
}

int ppf_noise_fit_rows(ppf_ctx* ctx, int32_t nrow, int32_t nbin, const double* in, double fact,
                       double* noise_out, int32_t* kc_out, int32_t* idx_out) {
  if (!ctx || !in || !noise_out) return fail(ctx, PPF_ERR_INVALID, "null argument");
  if (nrow <= 0) return PPF_OK;
  int logN;
  if (int r = check_nbin_any(ctx, nbin, &logN)) return r;
  if (!(fact > 0.0) || !std::isfinite(fact))
    return fail(ctx, PPF_ERR_INVALID, "fact=%g: must be positive and finite", fact);
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const double2* tw;
  if (int r = twiddles(ctx, nbin, &tw)) return r;
  return timed(ctx, PPF_K_NOISE, [&] {
    ROW_SWITCH(logN, nbin, hipLaunchKernelGGL(k_noise_fit_rows<Row>, dim3(nrow), dim3(kBlock),
                                              lds(kLdsSpec), ctx->stream, in, fact, noise_out,
                                              kc_out, idx_out, tw, row));
  });
}

int ppf_find_kc_rows(ppf_ctx* ctx, int32_t nrow, int32_t n, const double* pows,
                     const double* errs, int32_t fn, int32_t* kc_out, int32_t* idx_out) {
  if (!ctx || !pows || !kc_out) return fail(ctx, PPF_ERR_INVALID, "null argument");
  if (nrow <= 0) return PPF_OK;
  if (n < 4 || n > 8193)
    return fail(ctx, PPF_ERR_UNSUPPORTED, "n=%d: outside [4, 8193]", n);
  if (fn != 0 && fn != 1) return fail(ctx, PPF_ERR_INVALID, "fn=%d: 0 (exp_dc) or 1 (half_tri)", fn);
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const size_t lds = (size_t)n * sizeof(double);
  return timed(ctx, PPF_K_NOISE, [&] {
    if (fn == 0)
      hipLaunchKernelGGL(k_find_kc_rows<0>, dim3(nrow), dim3(kBlock), lds, ctx->stream, pows, errs,
                         n, kc_out, idx_out);
    else
      hipLaunchKernelGGL(k_find_kc_rows<1>, dim3(nrow), dim3(kBlock), lds, ctx->stream, pows, errs,
                         n, kc_out, idx_out);
  });
}

int ppf_synth_portraits(ppf_ctx* ctx, int32_t nsub, int32_t nchan, int32_t nbin,
                        const double* model, const double* phase, double sigma, uint64_t seed,
                        int64_t sub0, double* data) {
  if (!ctx || !model || !phase || !data) return fail(ctx, PPF_ERR_INVALID, "null argument");
  if (nsub <= 0 || nchan <= 0) return PPF_OK;
  int logN;
  if (int r = check_nbin_any(ctx, nbin, &logN)) return r;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  double2* M;
  double* pn;
  if (int r = model_spectra(ctx, nchan, nbin, model, 0, ctx->buf[kAux], &M, &pn)) return r;
  const double2* tw;
  if (int r = twiddles(ctx, nbin, &tw)) return r;
  const int NHP = nharm_pad(nbin);
  const int64_t rows = (int64_t)nsub * nchan;
  if (rows > 0x7fffffff) return fail(ctx, PPF_ERR_INVALID, "too many rows");
  return timed(ctx, PPF_K_SYNTH, [&] {
    ROW_SWITCH(logN, nbin, hipLaunchKernelGGL(k_synth<Row>, dim3((unsigned)rows), dim3(kBlock),
                                              lds(kLdsSpec), ctx->stream, M, phase, data, nchan,
                                              NHP, sigma, seed, sub0, tw, row));
  });
}

int ppf_pack_subints(ppf_ctx* ctx, int32_t nsub, int32_t npol, int32_t nchan, int32_t nbin,
                     const double* data, int16_t* raw, double* scl, double* offs) {
  if (!ctx || !data || !raw || !scl || !offs) return fail(ctx, PPF_ERR_INVALID, "null argument");
  if (nsub <= 0) return PPF_OK;
  if (npol <= 0 || nchan <= 0) return fail(ctx, PPF_ERR_INVALID, "bad shape");
  int logN;
  if (int r = check_nbin_any(ctx, nbin, &logN)) return r;
  const size_t rows = (size_t)nsub * npol * nchan;
  if (rows > 0x7fffffffULL) return fail(ctx, PPF_ERR_INVALID, "%zu profiles in one call", rows);
  HIPCHK(ctx, hipSetDevice(ctx->device));
  int* bad;
  if (int r = pack_begin(ctx, 0, &bad)) return r;
  if (int r = launch_pack(ctx, rows, nbin, data, raw, scl, offs, bad)) return r;
  return pack_end(ctx, bad);
}

int ppf_fake_subints(ppf_ctx* ctx, int32_t nsub, int32_t npol, int32_t nchan, int32_t nbin,
                     const double* model, const double* phase, const double* amp,
                     const double* sigma, uint64_t seed, int64_t sub0, double* data, int16_t* raw,
                     double* scl, double* offs) {
  if (!ctx || !model || !phase || !amp || !sigma) return fail(ctx, PPF_ERR_INVALID, "null argument");
  const bool pack = data == nullptr;
  if (pack ? (!raw || !scl || !offs) : (raw || scl || offs))
    return fail(ctx, PPF_ERR_INVALID, "pass data, or raw with scl and offs");
  if (nsub <= 0) return PPF_OK;
  if (npol <= 0 || nchan <= 0 || (int64_t)npol * nchan > 0x7fffffff)
    return fail(ctx, PPF_ERR_INVALID, "bad shape");
  int logN;
  if (int r = check_nbin_any(ctx, nbin, &logN)) return r;
  const size_t rows = (size_t)nsub * npol * nchan;
  if (rows > 0x7fffffffULL) return fail(ctx, PPF_ERR_INVALID, "%zu profiles in one call", rows);
  HIPCHK(ctx, hipSetDevice(ctx->device));
  double2* M;
  double* pn;
  if (int r = model_spectra(ctx, nchan, nbin, model, 0, ctx->buf[kAux], &M, &pn)) return r;
  const double2* tw;
  if (int r = twiddles(ctx, nbin, &tw)) return r;
  FakeArgs a{};
  a.M = M;
  a.phase = phase;
  a.amp = amp;
  a.sigma = sigma;
  a.npol = npol;
  a.nchan = nchan;
  a.NHP = nharm_pad(nbin);
  a.seed = seed;
  a.sub0 = sub0;
  a.data = data;
  a.raw = reinterpret_cast<short*>(raw);
  a.scl = scl;
  a.offs = offs;
  const bool fused = pack && logN >= 0;
  if (pack) {
    // generic nbin: the fp64 rows go through the workspace, then k_pack
    const size_t rbytes = fused ? 0 : rows * (size_t)nbin * sizeof(double);
    if ((int64_t)rbytes > ctx->ws_limit)
      return fail(ctx, PPF_ERR_NOMEM, "%zu bytes of rows exceed the workspace limit", rbytes);
    if (int r = pack_begin(ctx, rbytes, &a.bad)) return r;
    if (!fused) a.data = reinterpret_cast<double*>(static_cast<char*>(ctx->buf[kPack].p) + kPackHead);
  }
  if (int r = timed(ctx, PPF_K_SYNTH, [&] {
        if (fused) {  // power of two only
          LOGN_SWITCH(logN, hipLaunchKernelGGL((k_fake<RowPow2<LG>, true>), dim3((unsigned)rows),
                                               dim3(kBlock), 0, ctx->stream, a, tw,
                                               RowPow2<LG>{}));
        } else {
          ROW_SWITCH(logN, nbin, hipLaunchKernelGGL((k_fake<Row, false>), dim3((unsigned)rows),
                                                    dim3(kBlock), lds(kLdsSpec), ctx->stream, a,
                                                    tw, row));
        }
      }))
    return r;
  if (!pack) return PPF_OK;
  if (!fused)
    if (int r = launch_pack(ctx, rows, nbin, a.data, raw, scl, offs, a.bad)) return r;
  return pack_end(ctx, a.bad);
}

int ppf_rotate_accumulate(ppf_ctx* ctx, int32_t nsub, int32_t nchan, int32_t nbin,
                          const double* data, const double* phase, const double* weight,
                          double* accum) {
  if (!ctx || !data || !phase || !weight || !accum)
    return fail(ctx, PPF_ERR_INVALID, "null argument");
  if (nsub <= 0 || nchan <= 0) return PPF_OK;
  int logN;
  if (int r = check_nbin_any(ctx, nbin, &logN)) return r;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const double2* tw;
  if (int r = twiddles(ctx, nbin, &tw)) return r;
  const int NH = nbin / 2 + 1;
  // one workgroup per (slice, channel), about 2048 of them (8 per CU); nbin
  // 2048: four waves each streaming every fourth row of the slice (register
  // FFT), so a slice should hold a few groups of four
  const bool wave = logN == 10;
  int nsplit = (2048 + nchan - 1) / nchan;
  if (wave && nsplit > (nsub + 3) / 4) nsplit = (nsub + 3) / 4;
  if (nsplit > nsub) nsplit = nsub;
  if (nsplit < 1) nsplit = 1;
  const size_t count = (size_t)nchan * NH;
  if (int r = ensure(ctx, ctx->buf[kAux], (size_t)nsplit * count * sizeof(double2))) return r;
  double2* partial = reinterpret_cast<double2*>(ctx->buf[kAux].p);
  if (int r = timed(ctx, PPF_K_ROT_ACCUM, [&] {
        if (wave)
          hipLaunchKernelGGL(k_rot_accum_w, dim3(nsplit * nchan), dim3(256), 0,
                             ctx->stream, data, phase, weight, partial, nsub, nchan, nsplit, tw);
        else
          ROW_SWITCH(logN, nbin, hipLaunchKernelGGL(k_rot_accum<Row>, dim3(nsplit * nchan),
                                                    dim3(kBlock), lds(kLdsRow), ctx->stream, data,
                                                    phase, weight, partial, nsub, nchan, nsplit,
                                                    tw, row));
      }))
    return r;
  double2* acc = reinterpret_cast<double2*>(accum);
  return timed(ctx, PPF_K_ROT_ACCUM, [&] {
    hipLaunchKernelGGL(k_accum_reduce, dim3((unsigned)((count + 255) / 256)), dim3(256), 0,
                       ctx->stream, partial, acc, nsplit, count);
  });
}

int32_t ppf_spec_nhp(int32_t nbin) {
  int logN;
  if (check_nbin_any(nullptr, nbin, &logN)) return -1;
  return nharm_pad(nbin);
}

int ppf_rotate_accumulate_spec(ppf_ctx* ctx, int32_t nsub, int32_t nchan, int32_t nbin,
                               const double* spec, const double* phase, const double* weight,
                               double* accum) {
  if (!ctx || !spec || !phase || !weight || !accum)
    return fail(ctx, PPF_ERR_INVALID, "null argument");
  if (nsub <= 0 || nchan <= 0) return PPF_OK;
  int logN;
  if (int r = check_nbin_any(ctx, nbin, &logN)) return r;  // spectra of any length
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const int N = nbin / 2, NH = N + 1, NHP = nharm_pad(nbin);
  // one workgroup per (slice, channel), about 2048 of them (8 per CU)
  int nsplit = (2048 + nchan - 1) / nchan;
  if (nsplit > nsub) nsplit = nsub;
  if (nsplit < 1) nsplit = 1;
  const size_t count = (size_t)nchan * NH;
  if (int r = ensure(ctx, ctx->buf[kAux], (size_t)nsplit * count * sizeof(double2))) return r;
  double2* partial = reinterpret_cast<double2*>(ctx->buf[kAux].p);
  if (int r = timed(ctx, PPF_K_ROT_ACCUM, [&] {
        hipLaunchKernelGGL(k_rot_accum_spec, dim3(nsplit * nchan), dim3(256), 0, ctx->stream,
                           reinterpret_cast<const double2*>(spec), phase, weight, partial, nsub,
                           nchan, nsplit, N, NHP);
      }))
    return r;
  double2* acc = reinterpret_cast<double2*>(accum);
  return timed(ctx, PPF_K_ROT_ACCUM, [&] {
    hipLaunchKernelGGL(k_accum_reduce, dim3((unsigned)((count + 255) / 256)), dim3(256), 0,
                       ctx->stream, partial, acc, nsplit, count);
  });
}

int ppf_rotate_fscrunch(ppf_ctx* ctx, int32_t nunit, int32_t nchan, int32_t nbin,
                        const double* data, const double* phase, const double* weight,
                        double* prof) {
  if (!ctx || !data || !phase || !weight || !prof)
    return fail(ctx, PPF_ERR_INVALID, "null argument");
  if (nunit <= 0) return PPF_OK;
  int logN;
  if (int r = check_nbin_any(ctx, nbin, &logN)) return r;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  if (nchan <= 0) {  // an empty sum per unit
    HIPCHK(ctx, hipMemsetAsync(prof, 0, (size_t)nunit * nbin * sizeof(double), ctx->stream));
    return PPF_OK;
  }
  const double2* tw;
  if (int r = twiddles(ctx, nbin, &tw)) return r;
  const int NH = nbin / 2 + 1;
  // slices of kFsSlice channels whatever the call holds: a unit's profile
  // is summed in the same order alone or among others
  const int nslice = (nchan + kFsSlice - 1) / kFsSlice;
  // per unit: the slices' partial spectra, then the unit's spectrum; units in
  // chunks under the workspace limit (and one launch's grid)
  const size_t bPart = (size_t)nslice * NH * sizeof(double2), bSpec = (size_t)NH * sizeof(double2);
  const int64_t chunk = std::max<int64_t>(
      1, std::min<int64_t>({(int64_t)nunit, ctx->ws_limit / (int64_t)(bPart + bSpec + 512),
                            (int64_t)0x7fffffff / nslice}));
  const size_t oSpec = align256((size_t)chunk * bPart);
  if (int r = ensure(ctx, ctx->buf[kWs], oSpec + (size_t)chunk * bSpec)) return r;
  double2* partial = reinterpret_cast<double2*>(ctx->buf[kWs].p);
  double2* spec = reinterpret_cast<double2*>(static_cast<char*>(ctx->buf[kWs].p) + oSpec);
  const int nyq = (nbin & 1) ? -1 : nbin / 2;
  const bool wave = logN == 10;  // nbin 2048: the register FFT (2.6x the LDS kernel)
  for (int64_t u0 = 0; u0 < nunit; u0 += chunk) {
    const int nu = (int)std::min<int64_t>(chunk, nunit - u0);
    const double* d = data + (size_t)u0 * nchan * nbin;
    const double* ph = phase + (size_t)u0 * nchan;
    const double* w = weight + (size_t)u0 * nchan;
    const unsigned grid = (unsigned)nu * (unsigned)nslice;
    const size_t count = (size_t)nu * NH;
    if (int r = timed(ctx, PPF_K_FSCRUNCH, [&] {
          if (logN < 0)
            hipLaunchKernelGGL(k_fscrunch_gen, dim3(grid), dim3(kBlock),
                               RowAny::lds(nbin, kLdsRow), ctx->stream, d, ph, w, partial, nchan,
                               nslice, tw, RowAny{nbin});
          else if (wave)
            hipLaunchKernelGGL(k_fscrunch_w, dim3(grid), dim3(256), 0, ctx->stream, d, ph, w,
                               partial, nchan, nslice, tw);
          else
            LOGN_SWITCH(logN, hipLaunchKernelGGL(k_fscrunch<LG>, dim3(grid), dim3(kBlock), 0,
                                                 ctx->stream, d, ph, w, partial, nchan, nslice,
                                                 tw));
        }))
      return r;
    if (int r = timed(ctx, PPF_K_FSCRUNCH, [&] {
          hipLaunchKernelGGL(k_fscrunch_reduce, dim3((unsigned)((count + 255) / 256)), dim3(256),
                             0, ctx->stream, partial, spec, nslice, NH, nyq, count);
        }))
      return r;
    if (int r = timed(ctx, PPF_K_FSCRUNCH, [&] {
          launch_irfft_rows(ctx->stream, logN, nbin, nu, spec, prof + (size_t)u0 * nbin, tw);
        }))
      return r;
  }
  return PPF_OK;
}

int ppf_gaussian_portraits(ppf_ctx* ctx, int32_t nrow, int32_t nbin, int32_t ngauss,
                           const int32_t* code, const double* params, double nu_ref, double alpha,
                           const double* freqs, double* out) {
  if (!ctx || !code || !params || !freqs || !out) return fail(ctx, PPF_ERR_INVALID, "null argument");
  if (nrow <= 0) return PPF_OK;
  if (ngauss < 0 || ngauss > kMaxGauss)
    return fail(ctx, PPF_ERR_UNSUPPORTED, "ngauss=%d: at most %d components", ngauss, kMaxGauss);
  for (int i = 0; i < 3; ++i)
    if (code[i] != 0 && code[i] != 1)
      return fail(ctx, PPF_ERR_INVALID, "model code digit %d: 0 (power law) or 1 (linear)", code[i]);
  int logN;
  if (int r = check_nbin_any(ctx, nbin, &logN)) return r;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  GaussArgs g;
  g.nbin = nbin;
  g.ngauss = ngauss;
  for (int i = 0; i < 3; ++i) g.code[i] = code[i];
  // the constants numpy forms on the host (glibc log / sqrt, as numpy's)
  g.nu_ref = nu_ref;
  g.lnu = std::log(nu_ref);
  g.fwhm = 2.0 * std::sqrt(2.0 * std::log(2.0));
  g.sqrt2pi = std::sqrt(2.0 * M_PI);
  for (int i = 0; i < 2 + 6 * ngauss; ++i) g.params[i] = params[i];
  const bool scat = params[1] != 0.0;
  // gen_gaussian_portrait's scattering branch (pplib.py:915-922): unscattered
  // rows into a scratch buffer, then scattered into out
  double* rows = out;
  double* taus = nullptr;
  if (scat) {
    const size_t nb = (size_t)nrow * nbin;
    if (int r = ensure(ctx, ctx->buf[kAux], (nb + (size_t)nrow) * sizeof(double))) return r;
    rows = static_cast<double*>(ctx->buf[kAux].p);
    taus = rows + nb;
  }
  if (int r = timed(ctx, PPF_K_MODEL_FFT, [&] {
        hipLaunchKernelGGL(k_gauss_port, dim3(nrow), dim3(256), 0, ctx->stream, g, freqs, rows);
      }))
    return r;
  if (!scat) return PPF_OK;
  const double2* tw;
  if (int r = twiddles(ctx, nbin, &tw)) return r;
  return timed(ctx, PPF_K_MODEL_FFT, [&] {
    hipLaunchKernelGGL(k_scat_taus, dim3((nrow + 255) / 256), dim3(256), 0, ctx->stream, freqs,
                       nrow, params[1] / (double)nbin, alpha, nu_ref, taus);
    launch_rotate_rows(ctx->stream, logN, nbin, nrow, rows, nullptr, taus, out, tw);
  });
}

int ppf_unpack_subints(ppf_ctx* ctx, int32_t nsub, int32_t npol, int32_t nchan, int32_t nbin,
                       int32_t raw_type, const void* raw, const double* scl, const double* offs,
                       int32_t pmode, double* out) {
  if (!ctx || !raw || !scl || !offs || !out) return fail(ctx, PPF_ERR_INVALID, "null argument");
  if (nsub <= 0) return PPF_OK;
  if (npol <= 0 || nchan <= 0 || nbin <= 0) return fail(ctx, PPF_ERR_INVALID, "bad shape");
  if (raw_type < 1 || raw_type > 3) return fail(ctx, PPF_ERR_INVALID, "raw_type %d", raw_type);
  if (pmode < 0 || pmode > 2 || (pmode == 1 && npol < 2))
    return fail(ctx, PPF_ERR_INVALID, "pmode %d with npol %d", pmode, npol);
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const int npo = pmode ? 1 : npol;
  const size_t rows = (size_t)nsub * npo * nchan;
  if (rows > 0x7fffffffULL) return fail(ctx, PPF_ERR_INVALID, "%zu profiles in one call", rows);
  const dim3 g((unsigned)rows);
  return timed(ctx, PPF_K_UNPACK, [&] {
    switch (raw_type) {
      case 1:
        hipLaunchKernelGGL(k_unpack<uint8_t>, g, dim3(256), 0, ctx->stream,
                           static_cast<const uint8_t*>(raw), scl, offs, nsub, npol, nchan, nbin,
                           pmode, out);
        break;
      case 2:
        hipLaunchKernelGGL(k_unpack<int16_t>, g, dim3(256), 0, ctx->stream,
                           static_cast<const int16_t*>(raw), scl, offs, nsub, npol, nchan, nbin,
                           pmode, out);
        break;
      default:
        hipLaunchKernelGGL(k_unpack<float>, g, dim3(256), 0, ctx->stream,
                           static_cast<const float*>(raw), scl, offs, nsub, npol, nchan, nbin,
                           pmode, out);
    }
  });
}

int ppf_remove_baseline(ppf_ctx* ctx, int32_t nsub, int32_t npol, int32_t nchan, int32_t nbin,
                        int32_t ntot, int32_t width, double* data, const double* weights,
                        int32_t* window) {
  if (!ctx || !data || !weights) return fail(ctx, PPF_ERR_INVALID, "null argument");
  if (nsub <= 0) return PPF_OK;
  if (npol <= 0 || nchan <= 0 || nbin <= 0 || nbin > 8192)
    return fail(ctx, PPF_ERR_INVALID, "bad shape (%d, %d, %d)", npol, nchan, nbin);
  if (ntot < 1 || ntot > npol) return fail(ctx, PPF_ERR_INVALID, "ntot %d with npol %d", ntot, npol);
  if (width < 1 || width > nbin) return fail(ctx, PPF_ERR_INVALID, "width %d", width);
  HIPCHK(ctx, hipSetDevice(ctx->device));
  return timed(ctx, PPF_K_UNPACK, [&] {
    hipLaunchKernelGGL(k_remove_baseline, dim3(nsub), dim3(256), (size_t)nbin * sizeof(double),
                       ctx->stream, data, weights, npol, nchan, nbin, ntot, width, window);
  });
}

int ppf_profile_snr(ppf_ctx* ctx, int32_t nrow, int32_t nbin, const double* rows, int32_t width,
                    double threshold, double* out) {
  if (!ctx || !rows || !out) return fail(ctx, PPF_ERR_INVALID, "null argument");
  if (nrow <= 0) return PPF_OK;
  if (nbin <= 0 || nbin > 8192) return fail(ctx, PPF_ERR_INVALID, "nbin %d", nbin);
  if (width < 1 || width > nbin) return fail(ctx, PPF_ERR_INVALID, "width %d", width);
  if (!(threshold >= 0.0 && threshold < 0.5))
    return fail(ctx, PPF_ERR_INVALID, "threshold %g outside [0, 0.5)", threshold);
  HIPCHK(ctx, hipSetDevice(ctx->device));
  return timed(ctx, PPF_K_UNPACK, [&] {
    hipLaunchKernelGGL(k_profile_snr, dim3(nrow), dim3(64), (size_t)nbin * sizeof(double),
                       ctx->stream, rows, nbin, width, threshold, out);
  });
}

int ppf_resid_chi2_rows(ppf_ctx* ctx, int32_t nrow, int32_t nbin, const double* data,
                        const double* phase, const double* model, const int32_t* model_row,
                        const double* scale, const double* tau, const double* errs,
                        double dof, double* out) {
  if (!ctx || !data || !model || !scale || !errs || !out)
    return fail(ctx, PPF_ERR_INVALID, "null argument");
  if (nrow <= 0) return PPF_OK;
  if (!(dof > 0.0)) return fail(ctx, PPF_ERR_INVALID, "dof must be > 0");
  int logN;
  if (int r = check_nbin_any(ctx, nbin, &logN)) return r;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const double2* tw;
  if (int r = twiddles(ctx, nbin, &tw)) return r;
  ResidArgs ra{data, phase, model, model_row, scale, tau, errs, dof, out};
  return timed(ctx, PPF_K_RESID, [&] {
    ROW_SWITCH(logN, nbin, hipLaunchKernelGGL(k_resid_chi2<Row>, dim3(nrow), dim3(kBlock),
                                              lds(kLdsRowInv), ctx->stream, ra, tw, row));
  });
}

int ppf_pca_portraits(ppf_ctx* ctx, int32_t nport, int32_t nchan, int32_t nbin, const double* port,
                      const double* weights, int32_t ncomp, double* mean_prof, double* eigval,
                      double* eigvec, int32_t* info) {
  if (!ctx || !port || !weights || !mean_prof || !eigval || !eigvec || !info)
    return fail(ctx, PPF_ERR_INVALID, "null argument");
  if (nport <= 0) return PPF_OK;
  int logN;
  if (int r = check_nbin_any(ctx, nbin, &logN)) return r;
  if (nchan < 2) return fail(ctx, PPF_ERR_INVALID, "nchan=%d: a PCA needs at least 2 rows", nchan);
  if (nchan > kPcaMaxRows)
    return fail(ctx, PPF_ERR_UNSUPPORTED, "nchan=%d: at most %d rows per portrait", nchan,
                kPcaMaxRows);
  if (ncomp < 1 || ncomp > std::min(nchan, nbin))
    return fail(ctx, PPF_ERR_INVALID, "ncomp=%d: 1..min(nchan, nbin)=%d", ncomp,
                std::min(nchan, nbin));
  HIPCHK(ctx, hipSetDevice(ctx->device));
  // the weights are checked on the host: fact = sum w - sum w^2 / sum w must be > 0
  std::vector<double> hw((size_t)nport * nchan);
  HIPCHK(ctx, hipMemcpyAsync(hw.data(), weights, hw.size() * sizeof(double), hipMemcpyDeviceToHost,
                             ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  for (int p = 0; p < nport; ++p) {
    int npos = 0;
    for (int n = 0; n < nchan; ++n) {
      const double w = hw[(size_t)p * nchan + n];
      if (!std::isfinite(w) || w < 0.0)
        return fail(ctx, PPF_ERR_INVALID, "portrait %d: weight %d is %g (need finite, >= 0)", p, n,
                    w);
      npos += w > 0.0;
    }
    if (npos < 2)
      return fail(ctx, PPF_ERR_INVALID, "portrait %d: %d positive weights (need at least 2)", p,
                  npos);
  }
  // per portrait: A [nchan][nbin], |row|^2 [nchan], the state, the order [ncomp]
  const int m = nchan, M = (m + 1) & ~1;
  const size_t bA = (size_t)m * nbin * sizeof(double), bN = (size_t)m * sizeof(double);
  const size_t bO = (size_t)ncomp * sizeof(int);
  const size_t per_port = bA + bN + sizeof(PcaState) + bO;
  // portraits per pass: under the workspace limit and the grid's y extent
  const int64_t chunk = std::max<int64_t>(
      1, std::min<int64_t>({(int64_t)nport, ctx->ws_limit / (int64_t)(per_port + 1024), 65535}));
  const size_t oN = align256((size_t)chunk * bA), oS = align256(oN + (size_t)chunk * bN);
  const size_t oO = align256(oS + (size_t)chunk * sizeof(PcaState));
  if (int r = ensure(ctx, ctx->buf[kWs], oO + (size_t)chunk * bO)) return r;
  char* base = static_cast<char*>(ctx->buf[kWs].p);
  double* A = reinterpret_cast<double*>(base);
  double* norm2 = reinterpret_cast<double*>(base + oN);
  PcaState* state = reinterpret_cast<PcaState*>(base + oS);
  int* order = reinterpret_cast<int*>(base + oO);
  std::vector<PcaState> hs((size_t)chunk);
  for (int64_t p0 = 0; p0 < nport; p0 += chunk) {
    const int np = (int)std::min<int64_t>(chunk, nport - p0);
    HIPCHK(ctx, hipMemsetAsync(state, 0, (size_t)np * sizeof(PcaState), ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(order, 0, (size_t)np * bO, ctx->stream));
    if (int r = timed(ctx, PPF_K_PCA, [&] {
          hipLaunchKernelGGL(k_pca_center, dim3((nbin + kBlock - 1) / kBlock, np), dim3(kBlock), 0,
                             ctx->stream, port + (size_t)p0 * m * nbin, weights + (size_t)p0 * m,
                             m, nbin, mean_prof + (size_t)p0 * nbin, A);
        }))
      return r;
    // the host reads the portraits' states once per sweep and stops when
    // every one is done (converged, or kPcaMaxSweeps sweeps made)
    for (int sweep = 0; sweep <= kPcaMaxSweeps; ++sweep) {
      if (int r = timed(ctx, PPF_K_PCA, [&] {
            hipLaunchKernelGGL(k_pca_norms, dim3(m, np), dim3(kBlock), 0, ctx->stream, A, m, nbin,
                               norm2);
            hipLaunchKernelGGL(k_pca_sweep, dim3(np), dim3(kBlock), 0, ctx->stream, state, norm2,
                               m, nbin, sweep, kPcaMaxSweeps);
          }))
        return r;
      HIPCHK(ctx, hipMemcpyAsync(hs.data(), state, (size_t)np * sizeof(PcaState),
                                 hipMemcpyDeviceToHost, ctx->stream));
      HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
      bool all_done = true;
      for (int p = 0; p < np; ++p) all_done = all_done && hs[p].done != 0;
      if (all_done) break;
      if (int r = timed(ctx, PPF_K_PCA, [&] {
            for (int round = 0; round < M - 1; ++round)
              hipLaunchKernelGGL(k_pca_step, dim3(M / 2, np), dim3(kBlock), 0, ctx->stream, A,
                                 state, m, M, nbin, round);
          }))
        return r;
    }
    // (norm2 holds the final rows' norms: a done portrait is not rotated again)
    if (int r = timed(ctx, PPF_K_PCA, [&] {
          hipLaunchKernelGGL(k_pca_rank, dim3(np), dim3(kBlock), bN, ctx->stream, norm2, m, ncomp,
                             order);
          hipLaunchKernelGGL(k_pca_emit, dim3(ncomp, np), dim3(kBlock), 0, ctx->stream, A, norm2,
                             order, state, m, nbin, ncomp, eigval + (size_t)p0 * ncomp,
                             eigvec + (size_t)p0 * ncomp * nbin, info + (size_t)p0 * 2);
        }))
      return r;
  }
  return PPF_OK;
}

int ppf_pca_gram_portraits(ppf_ctx* ctx, int32_t nport, int32_t nchan, int32_t nbin,
                           const double* port, const double* weights, int32_t ncomp,
                           double* mean_prof, double* eigval, double* eigvec, int32_t* info) {
  if (!ctx || !port || !weights || !mean_prof || !eigval || !eigvec || !info)
    return fail(ctx, PPF_ERR_INVALID, "null argument");
  if (nport <= 0) return PPF_OK;
  int logN;
  if (int r = check_nbin_any(ctx, nbin, &logN)) return r;
  if (nbin > kPcaMaxRows)
    return fail(ctx, PPF_ERR_UNSUPPORTED, "nbin=%d: the covariance has at most %d rows", nbin,
                kPcaMaxRows);
  if (nchan < 2) return fail(ctx, PPF_ERR_INVALID, "nchan=%d: a PCA needs at least 2 rows", nchan);
  if (nchan > PPF_MAX_NCHAN)
    return fail(ctx, PPF_ERR_UNSUPPORTED, "nchan=%d: at most %d channels per portrait", nchan,
                PPF_MAX_NCHAN);
  if (ncomp < 1 || ncomp > std::min(nchan, nbin))
    return fail(ctx, PPF_ERR_INVALID, "ncomp=%d: 1..min(nchan, nbin)=%d", ncomp,
                std::min(nchan, nbin));
  HIPCHK(ctx, hipSetDevice(ctx->device));
  // the weights are checked on the host, as ppf_pca_portraits checks them
  std::vector<double> hw((size_t)nport * nchan);
  HIPCHK(ctx, hipMemcpyAsync(hw.data(), weights, hw.size() * sizeof(double), hipMemcpyDeviceToHost,
                             ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  for (int p = 0; p < nport; ++p) {
    int npos = 0;
    for (int n = 0; n < nchan; ++n) {
      const double w = hw[(size_t)p * nchan + n];
      if (!std::isfinite(w) || w < 0.0)
        return fail(ctx, PPF_ERR_INVALID, "portrait %d: weight %d is %g (need finite, >= 0)", p, n,
                    w);
      npos += w > 0.0;
    }
    if (npos < 2)
      return fail(ctx, PPF_ERR_INVALID, "portrait %d: %d positive weights (need at least 2)", p,
                  npos);
  }
  // per portrait: G [nbin][nbin], the slabs' partial tiles, the row scales
  // [nchan], |row|^2 [nbin], trace(G), the state, the order [ncomp]
  const int m = nbin, M = (m + 1) & ~1;
  const int npair = gram_npair(nbin), nslab = gram_nslab(nchan);
  const size_t bG = (size_t)m * nbin * sizeof(double), bN = (size_t)m * sizeof(double);
  const size_t bP = (size_t)nslab * npair * kGramTile * kGramTile * sizeof(double);
  const size_t bC = (size_t)nchan * sizeof(double), bO = (size_t)ncomp * sizeof(int);
  const size_t per_port = bG + bP + bC + bN + sizeof(double) + sizeof(PcaState) + bO;
  // portraits per pass: under the workspace limit and the grid's z extent
  const int64_t chunk = std::max<int64_t>(
      1, std::min<int64_t>({(int64_t)nport, ctx->ws_limit / (int64_t)(per_port + 2048), 65535}));
  const size_t oP = align256((size_t)chunk * bG), oC = align256(oP + (size_t)chunk * bP);
  const size_t oN = align256(oC + (size_t)chunk * bC), oT = align256(oN + (size_t)chunk * bN);
  const size_t oS = align256(oT + (size_t)chunk * sizeof(double));
  const size_t oO = align256(oS + (size_t)chunk * sizeof(PcaState));
  if (int r = ensure(ctx, ctx->buf[kWs], oO + (size_t)chunk * bO)) return r;
  char* base = static_cast<char*>(ctx->buf[kWs].p);
  double* G = reinterpret_cast<double*>(base);
  double* part = reinterpret_cast<double*>(base + oP);
  double* scale = reinterpret_cast<double*>(base + oC);
  double* norm2 = reinterpret_cast<double*>(base + oN);
  double* trace = reinterpret_cast<double*>(base + oT);
  PcaState* state = reinterpret_cast<PcaState*>(base + oS);
  int* order = reinterpret_cast<int*>(base + oO);
  std::vector<PcaState> hs((size_t)chunk);
  // under timing, the device time of the launches since the last mark goes to phase i
  double seen = 0.0;
  auto mark = [&](int i) -> int {
    if (!ctx->timing) return PPF_OK;
    if (int r = resolve_timing(ctx)) return r;
    if (i >= 0) ctx->gram_ms[i] += ctx->ktime[PPF_K_PCA] - seen;
    seen = ctx->ktime[PPF_K_PCA];
    return PPF_OK;
  };
  if (int r = mark(-1)) return r;
  for (int64_t p0 = 0; p0 < nport; p0 += chunk) {
    const int np = (int)std::min<int64_t>(chunk, nport - p0);
    const double* x = port + (size_t)p0 * nchan * nbin;
    double* mean = mean_prof + (size_t)p0 * nbin;
    HIPCHK(ctx, hipMemsetAsync(state, 0, (size_t)np * sizeof(PcaState), ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(order, 0, (size_t)np * bO, ctx->stream));
    if (int r = timed(ctx, PPF_K_PCA, [&] {
          hipLaunchKernelGGL(k_gram_mean, dim3((nbin + 63) / 64, np), dim3(64), 0, ctx->stream, x,
                             weights + (size_t)p0 * nchan, nchan, nbin, mean, scale);
        }))
      return r;
    if (int r = mark(0)) return r;
    if (int r = timed(ctx, PPF_K_PCA, [&] {
          hipLaunchKernelGGL(k_gram_tiles, dim3(gram_nsuper(nbin), nslab, np), dim3(kBlock), 0,
                             ctx->stream, x, scale, mean, nchan, nbin, npair, part);
        }))
      return r;
    if (int r = mark(1)) return r;
    if (int r = timed(ctx, PPF_K_PCA, [&] {
          hipLaunchKernelGGL(k_gram_reduce, dim3(npair, kGramTile / 4, np), dim3(kBlock), 0,
                             ctx->stream, part, nbin, nslab, G);
          hipLaunchKernelGGL(k_gram_trace, dim3(np), dim3(kBlock), 0, ctx->stream, G, nbin, trace);
        }))
      return r;
    if (int r = mark(2)) return r;
    // the Jacobi of ppf_pca_portraits on G's rows, with G's own null threshold
    for (int sweep = 0; sweep <= kPcaMaxSweeps; ++sweep) {
      if (int r = timed(ctx, PPF_K_PCA, [&] {
            hipLaunchKernelGGL(k_pca_norms, dim3(m, np), dim3(kBlock), 0, ctx->stream, G, m, nbin,
                               norm2);
            hipLaunchKernelGGL(k_pca_sweep, dim3(np), dim3(kBlock), 0, ctx->stream, state, norm2,
                               m, nbin, sweep, kPcaMaxSweeps);
            hipLaunchKernelGGL(k_gram_null, dim3((np + kBlock - 1) / kBlock), dim3(kBlock), 0,
                               ctx->stream, state, trace, nchan, np);
          }))
        return r;
      HIPCHK(ctx, hipMemcpyAsync(hs.data(), state, (size_t)np * sizeof(PcaState),
                                 hipMemcpyDeviceToHost, ctx->stream));
      HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
      bool all_done = true;
      for (int p = 0; p < np; ++p) all_done = all_done && hs[p].done != 0;
      if (all_done) break;
      if (int r = timed(ctx, PPF_K_PCA, [&] {
            for (int round = 0; round < M - 1; ++round)
              hipLaunchKernelGGL(k_pca_step, dim3(M / 2, np), dim3(kBlock), 0, ctx->stream, G,
                                 state, m, M, nbin, round);
          }))
        return r;
    }
    if (int r = mark(3)) return r;
    if (int r = timed(ctx, PPF_K_PCA, [&] {
          hipLaunchKernelGGL(k_pca_rank, dim3(np), dim3(kBlock), bN, ctx->stream, norm2, m, ncomp,
                             order);
          hipLaunchKernelGGL(k_pca_emit, dim3(ncomp, np), dim3(kBlock), 0, ctx->stream, G, norm2,
                             order, state, m, nbin, ncomp, eigval + (size_t)p0 * ncomp,
                             eigvec + (size_t)p0 * ncomp * nbin, info + (size_t)p0 * 2);
          hipLaunchKernelGGL(k_gram_sqrt, dim3((np * ncomp + kBlock - 1) / kBlock), dim3(kBlock),
                             0, ctx->stream, eigval + (size_t)p0 * ncomp, np * ncomp);
        }))
      return r;
    if (int r = mark(4)) return r;
  }
  return PPF_OK;
}

int ppf_pca_project(ppf_ctx* ctx, int32_t nport, int32_t nchan, int32_t nbin, const double* port,
                    const double* mean_prof, int32_t ncomp, const double* eigvec, double* proj,
                    double* reconst) {
  if (!ctx || !port || !mean_prof || !eigvec || !proj)
    return fail(ctx, PPF_ERR_INVALID, "null argument");
  if (nport <= 0) return PPF_OK;
  int logN;
  if (int r = check_nbin_any(ctx, nbin, &logN)) return r;
  if (nchan < 1) return fail(ctx, PPF_ERR_INVALID, "nchan=%d", nchan);
  if (nchan > PPF_MAX_NCHAN)
    return fail(ctx, PPF_ERR_UNSUPPORTED, "nchan=%d: at most %d channels per portrait", nchan,
                PPF_MAX_NCHAN);
  if (ncomp < 1 || ncomp > std::min<int>(kPcaMaxRows, nbin))
    return fail(ctx, PPF_ERR_INVALID, "ncomp=%d: 1..%d", ncomp, std::min<int>(kPcaMaxRows, nbin));
  HIPCHK(ctx, hipSetDevice(ctx->device));
  for (int64_t p0 = 0; p0 < nport; p0 += 65535) {  // the grid's y extent
    const int np = (int)std::min<int64_t>(65535, nport - p0);
    if (int r = timed(ctx, PPF_K_PCA, [&] {
          hipLaunchKernelGGL(k_pca_project, dim3(nchan, np), dim3(kBlock),
                             (size_t)ncomp * sizeof(double), ctx->stream,
                             port + (size_t)p0 * nchan * nbin, mean_prof + (size_t)p0 * nbin,
                             eigvec + (size_t)p0 * ncomp * nbin, nchan, nbin, ncomp,
                             proj + (size_t)p0 * nchan * ncomp,
                             reconst ? reconst + (size_t)p0 * nchan * nbin : nullptr);
        }))
      return r;
  }
  return PPF_OK;
}

}  // extern "C"

namespace {

// SWT_SWITCH: LG = log2(nbin / 2) of the FFT kernels' lengths, 0 for any
// other nbin (the generic-length sums)
#define SWT_SWITCH(L, ...)                                 \
  switch (L) {                                             \
    case 5: { constexpr int LG = 5; __VA_ARGS__; } break;    \
    case 6: { constexpr int LG = 6; __VA_ARGS__; } break;    \
    case 7: { constexpr int LG = 7; __VA_ARGS__; } break;    \
    case 8: { constexpr int LG = 8; __VA_ARGS__; } break;    \
    case 9: { constexpr int LG = 9; __VA_ARGS__; } break;    \
    case 10: { constexpr int LG = 10; __VA_ARGS__; } break;  \
    case 11: { constexpr int LG = 11; __VA_ARGS__; } break;  \
    case 12: { constexpr int LG = 12; __VA_ARGS__; } break;  \
    default: { constexpr int LG = 0; __VA_ARGS__; } break;   \
  }

// One pass of the wavelet entry points over rows [r0, r0 + nr): the forward
// transform, the medians and the rows' noise into the workspace, then `work`.
struct SwtPlan {
  int64_t chunk;
  size_t oMed, oNz, oNoise, oGrid, oPf, oPv, total;
  SwtPlan(int nbin, int L, int64_t nrow, int64_t ws_limit) {
    const size_t perW = (size_t)L * 2 * nbin * sizeof(double);
    const size_t per_row = perW + (size_t)L * (3 + kSwtGrid) * sizeof(double) + 16;
    chunk = std::max<int64_t>(
        1, std::min<int64_t>({nrow, ws_limit / (int64_t)(per_row + 64), 65535}));
    oMed = align256((size_t)chunk * perW);
    oNz = align256(oMed + (size_t)chunk * L * sizeof(double));
    oNoise = align256(oNz + (size_t)chunk * sizeof(int));
    oGrid = align256(oNoise + (size_t)chunk * sizeof(double));
    oPf = align256(oGrid + (size_t)chunk * L * kSwtGrid * sizeof(double));
    oPv = align256(oPf + (size_t)chunk * L * sizeof(double));
    total = oPv + (size_t)chunk * L * sizeof(double);
  }
  void bind(SwtArgs& a, void* ws) const {
    char* base = static_cast<char*>(ws);
    a.W = reinterpret_cast<double*>(base);
    a.med = reinterpret_cast<double*>(base + oMed);
    a.nz = reinterpret_cast<int*>(base + oNz);
    a.noise = reinterpret_cast<double*>(base + oNoise);
    a.fgrid = reinterpret_cast<double*>(base + oGrid);
    a.pfact = reinterpret_cast<double*>(base + oPf);
    a.pfun = reinterpret_cast<double*>(base + oPv);
  }
};

// nbin even in [16, 8192]; every level in 1 .. 13 with nbin divisible by
// 2^level (pywt.swt's condition)
int swt_check(ppf_ctx* ctx, int nbin, int threshtype, int* logN) {
  if (int r = check_nbin_any(ctx, nbin, logN)) return r;
  if (nbin & 1)
    return fail(ctx, PPF_ERR_UNSUPPORTED, "nbin=%d: the transform needs an even nbin", nbin);
  if (threshtype != PPF_THRESH_HARD && threshtype != PPF_THRESH_SOFT)
    return fail(ctx, PPF_ERR_INVALID, "threshtype=%d: PPF_THRESH_HARD or PPF_THRESH_SOFT",
                threshtype);
  return PPF_OK;
}
int swt_check_level(ppf_ctx* ctx, int nbin, int level) {
  if (level < 1 || level > 13 || nbin % (1 << level))
    return fail(ctx, PPF_ERR_INVALID, "nlevel=%d: 1..13 with nbin=%d a multiple of 2^nlevel", level,
                nbin);
  return PPF_OK;
}

// the per-row levels on the host, checked; *L their maximum
int swt_row_levels(ppf_ctx* ctx, int nrow, int nbin, const int32_t* nlevel, int* L) {
  std::vector<int32_t> h((size_t)nrow);
  HIPCHK(ctx, hipMemcpyAsync(h.data(), nlevel, h.size() * sizeof(int32_t), hipMemcpyDeviceToHost,
                             ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  *L = 0;
  for (int r = 0; r < nrow; ++r) {
    if (int e = swt_check_level(ctx, nbin, h[r])) return e;
    *L = std::max(*L, (int)h[r]);
  }
  return PPF_OK;
}

void swt_base_args(SwtArgs& a, int nbin, int L, int threshtype, double tol, const double2* tw) {
  std::memset(&a, 0, sizeof(a));
  a.nbin = nbin;
  a.L = L;
  a.soft = threshtype == PPF_THRESH_SOFT;
  a.kc = noise_kc(nbin);
  a.tol = tol;
  a.sq2ln = std::sqrt(2.0 * std::log((double)nbin));
  a.tw = tw;
}

// forward transform, medians (deepest: only each row's deepest level) and,
// with noise, get_noise_PS of the nr rows a.rows
void swt_launch_forward(ppf_ctx* ctx, const SwtArgs& a, int nr, int logN, int deepest, bool noise) {
  const size_t lds = 2 * (size_t)a.nbin * sizeof(double);
  hipLaunchKernelGGL(k_swt_forward, dim3(nr), dim3(kBlock), lds, ctx->stream, a);
  hipLaunchKernelGGL(k_swt_median, dim3(a.L, nr), dim3(kBlock), 0, ctx->stream, a, deepest);
  if (!noise) return;
  double* out = const_cast<double*>(a.noise);
  ROW_SWITCH(logN, a.nbin, hipLaunchKernelGGL(k_noise_rows<Row>, dim3(nr), dim3(kBlock),
                                              lds(kLdsRow), ctx->stream, a.rows, out, a.kc, a.tw,
                                              row));
}

}  // namespace

extern "C" {

int ppf_wavelet_smooth_rows(ppf_ctx* ctx, int32_t nrow, int32_t nbin, const double* rows,
                            const int32_t* nlevel, const double* fact, int32_t threshtype,
                            double* out) {
  if (!ctx || !rows || !nlevel || !fact || !out) return fail(ctx, PPF_ERR_INVALID, "null argument");
  if (nrow <= 0) return PPF_OK;
  int logN, L;
  if (int r = swt_check(ctx, nbin, threshtype, &logN)) return r;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  if (int r = swt_row_levels(ctx, nrow, nbin, nlevel, &L)) return r;
  const double2* tw;
  if (int r = twiddles(ctx, nbin, &tw)) return r;
  const SwtPlan plan(nbin, L, nrow, ctx->ws_limit);
  if (int r = ensure(ctx, ctx->buf[kWs], plan.total)) return r;
  const size_t lds = 2 * (size_t)nbin * sizeof(double);
  for (int64_t r0 = 0; r0 < nrow; r0 += plan.chunk) {
    const int nr = (int)std::min<int64_t>(plan.chunk, nrow - r0);
    SwtArgs a;
    swt_base_args(a, nbin, L, threshtype, 0.0, tw);
    plan.bind(a, ctx->buf[kWs].p);
    a.rows = rows + (size_t)r0 * nbin;
    a.nlev = nlevel + r0;
    a.fact = fact + r0;
    a.out = out + (size_t)r0 * nbin;
    if (int r = timed(ctx, PPF_K_SWT, [&] {
          swt_launch_forward(ctx, a, nr, logN, 1, false);
          hipLaunchKernelGGL(k_swt_smooth, dim3(nr), dim3(kBlock), lds, ctx->stream, a, 0);
        }))
      return r;
  }
  return PPF_OK;
}

int ppf_wavelet_objective_rows(ppf_ctx* ctx, int32_t nrow, int32_t nbin, const double* rows,
                               const int32_t* nlevel, const double* fact, int32_t threshtype,
                               double rchi2_tol, double* obj, double* red_chi2) {
  if (!ctx || !rows || !nlevel || !fact || !obj || !red_chi2)
    return fail(ctx, PPF_ERR_INVALID, "null argument");
  if (nrow <= 0) return PPF_OK;
  int logN, L;
  if (int r = swt_check(ctx, nbin, threshtype, &logN)) return r;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  if (int r = swt_row_levels(ctx, nrow, nbin, nlevel, &L)) return r;
  const double2* tw;
  if (int r = twiddles(ctx, nbin, &tw)) return r;
  const SwtPlan plan(nbin, L, nrow, ctx->ws_limit);
  if (int r = ensure(ctx, ctx->buf[kWs], plan.total)) return r;
  const size_t lds = 2 * (size_t)nbin * sizeof(double);
  for (int64_t r0 = 0; r0 < nrow; r0 += plan.chunk) {
    const int nr = (int)std::min<int64_t>(plan.chunk, nrow - r0);
    SwtArgs a;
    swt_base_args(a, nbin, L, threshtype, rchi2_tol, tw);
    plan.bind(a, ctx->buf[kWs].p);
    a.rows = rows + (size_t)r0 * nbin;
    a.nlev = nlevel + r0;
    a.fact = fact + r0;
    a.o_obj = obj + r0;
    a.o_rchi2 = red_chi2 + r0;
    if (int r = timed(ctx, PPF_K_SWT, [&] {
          swt_launch_forward(ctx, a, nr, logN, 1, true);
          SWT_SWITCH(logN, hipLaunchKernelGGL(k_swt_objective<LG>, dim3(1, 1, nr), dim3(kBlock),
                                              lds, ctx->stream, a, 1));
        }))
      return r;
  }
  return PPF_OK;
}

int ppf_smart_smooth_rows(ppf_ctx* ctx, int32_t nrow, int32_t nbin, const double* rows,
                          int32_t try_nlevels, double rchi2_tol, int32_t threshtype, double* out,
                          int32_t* nlevel, double* fact, double* red_chi2, int32_t* zeroed,
                          double* table) {
  if (!ctx || !rows || !out || !nlevel || !fact || !red_chi2 || !zeroed)
    return fail(ctx, PPF_ERR_INVALID, "null argument");
  if (nrow <= 0) return PPF_OK;
  int logN;
  if (int r = swt_check(ctx, nbin, threshtype, &logN)) return r;
  if (int r = swt_check_level(ctx, nbin, try_nlevels)) return r;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const int L = try_nlevels;
  const double2* tw;
  if (int r = twiddles(ctx, nbin, &tw)) return r;
  const SwtPlan plan(nbin, L, nrow, ctx->ws_limit);
  if (int r = ensure(ctx, ctx->buf[kWs], plan.total)) return r;
  const size_t lds = 2 * (size_t)nbin * sizeof(double);
  for (int64_t r0 = 0; r0 < nrow; r0 += plan.chunk) {
    const int nr = (int)std::min<int64_t>(plan.chunk, nrow - r0);
    SwtArgs a;
    swt_base_args(a, nbin, L, threshtype, rchi2_tol, tw);
    plan.bind(a, ctx->buf[kWs].p);
    a.rows = rows + (size_t)r0 * nbin;
    a.out = out + (size_t)r0 * nbin;
    a.o_nlevel = nlevel + r0;
    a.o_fact = fact + r0;
    a.o_rchi2 = red_chi2 + r0;
    a.o_zeroed = zeroed + r0;
    // (an all-zero row is skipped by the search: its table entries stay 0)
    HIPCHK(ctx, hipMemsetAsync(a.pfun, 0, (size_t)nr * L * sizeof(double), ctx->stream));
    if (int r = timed(ctx, PPF_K_SWT, [&] {
          swt_launch_forward(ctx, a, nr, logN, 0, true);
          SWT_SWITCH(logN, hipLaunchKernelGGL(k_swt_objective<LG>, dim3(kSwtGrid, L, nr),
                                              dim3(kBlock), lds, ctx->stream, a, 0));
          SWT_SWITCH(logN, hipLaunchKernelGGL(k_swt_polish<LG>, dim3(L, nr), dim3(kBlock), lds,
                                              ctx->stream, a));
          hipLaunchKernelGGL(k_swt_smooth, dim3(nr), dim3(kBlock), lds, ctx->stream, a, 1);
        }))
      return r;
    if (table)
      HIPCHK(ctx, hipMemcpyAsync(table + (size_t)r0 * L, a.pfun, (size_t)nr * L * sizeof(double),
                                 hipMemcpyDeviceToDevice, ctx->stream));
  }
  return PPF_OK;
}

}  // extern "C"

namespace {

// Shapes of a Gaussian-component fit and the slices of its workspace, for
// `chunk` portraits (ppfit_gauss.hip).
struct GaussPlan {
  int npar, KT, KB, npairs, NH, logN;
  int64_t chunk;
  size_t oRows, oSpec, oDspec, oCoef, oTaun, oGram, oPext, oLm, oState, oBad, total;
};

// njoin < 0: no join parameters (one receiver)
int gauss_plan(ppf_ctx* ctx, int nport, int nchan, int nbin, int ngauss, int njoin, bool fit,
               GaussPlan* g) {
  if (ngauss < 1 || ngauss > kFitMaxGauss)
    return fail(ctx, PPF_ERR_UNSUPPORTED, "ngauss=%d: 1..%d components in a fit", ngauss,
                kFitMaxGauss);
  const bool join = njoin >= 0;
  if (join && (njoin < 1 || njoin > kFitMaxJoin))
    return fail(ctx, PPF_ERR_UNSUPPORTED, "njoin=%d: 1..%d join groups in a fit", njoin,
                kFitMaxJoin);
  if (join && 3 + 6 * ngauss + 2 * njoin > kGfMaxPar)
    return fail(ctx, PPF_ERR_UNSUPPORTED,
                "ngauss=%d, njoin=%d: 3 + 6 ngauss + 2 njoin = %d parameters, at most %d", ngauss,
                njoin, 3 + 6 * ngauss + 2 * njoin, kGfMaxPar);
  if (nchan < 1 || nchan > kFitMaxChan)
    return fail(ctx, PPF_ERR_UNSUPPORTED, "nchan=%d: 1..%d channels in a fit", nchan, kFitMaxChan);
  const int l = ilog2_exact(nbin);
  if (l < 6 || nbin > 8192)
    return fail(ctx, PPF_ERR_UNSUPPORTED, "nbin=%d: a power of two in [64, 8192]", nbin);
  g->logN = l - 1;
  g->npar = 3 + 6 * ngauss + (join ? 2 * njoin : 0);
  g->KT = 1 + 3 * ngauss;
  g->KB = g->KT + 2 + (join ? 1 : 0);
  g->npairs = g->KB * (g->KB + 1) / 2;
  g->NH = nbin / 2 + 1;
  const size_t rows = (size_t)nchan;
  const size_t bRows = rows * g->KT * nbin * sizeof(double);
  const size_t bSpec = rows * g->KT * g->NH * sizeof(double2);
  const size_t bDspec = rows * g->NH * sizeof(double2);
  const size_t bCoef = rows * g->npar * sizeof(double), bTaun = rows * sizeof(double);
  const size_t bGram = rows * g->npairs * sizeof(double), bPext = (size_t)g->npar * sizeof(double);
  const size_t bLm = fit ? (size_t)kGfLmDoubles * sizeof(double) : 0;
  const size_t per_port = bRows + bSpec + bDspec + bCoef + bTaun + bGram + bPext + bLm +
                          sizeof(GaussFitState);
  const int64_t chunk = std::max<int64_t>(
      1, std::min<int64_t>({(int64_t)nport, ctx->ws_limit / (int64_t)(per_port + 4096), 65535}));
  g->chunk = chunk;
  const size_t c = (size_t)chunk;
  g->oRows = 0;
  g->oSpec = align256(g->oRows + c * bRows);
  g->oDspec = align256(g->oSpec + c * bSpec);
  g->oCoef = align256(g->oDspec + c * bDspec);
  g->oTaun = align256(g->oCoef + c * bCoef);
  g->oGram = align256(g->oTaun + c * bTaun);
  g->oPext = align256(g->oGram + c * bGram);
  g->oLm = align256(g->oPext + c * bPext);
  g->oState = align256(g->oLm + c * bLm);
  g->total = g->oState + c * sizeof(GaussFitState);
  g->oBad = g->total;
  if (join) g->total = g->oBad + 256;  // the flag of k_gauss_join_check
  return PPF_OK;
}

void gauss_args(const GaussPlan& g, char* base, int nchan, int nbin, int ngauss, int njoin,
                GaussFitArgs* a) {
  a->nchan = nchan;
  a->nbin = nbin;
  a->ngauss = ngauss;
  a->npar = g.npar;
  a->njoin = njoin > 0 ? njoin : 0;
  a->join_of = nullptr;
  a->dm_coef = nullptr;
  a->max_nfev = 0;
  a->fwhm = 2.0 * std::sqrt(2.0 * std::log(2.0));
  a->sqrt2pi = std::sqrt(2.0 * M_PI);
  a->wid_max = 0.25;
  a->ftol = a->xtol = 0.0;
  a->rows = reinterpret_cast<double*>(base + g.oRows);
  a->spec = reinterpret_cast<double2*>(base + g.oSpec);
  a->dspec = reinterpret_cast<double2*>(base + g.oDspec);
  a->coef = reinterpret_cast<double*>(base + g.oCoef);
  a->taun = reinterpret_cast<double*>(base + g.oTaun);
  a->gram = reinterpret_cast<double*>(base + g.oGram);
  a->pext = reinterpret_cast<double*>(base + g.oPext);
  a->lm = reinterpret_cast<double*>(base + g.oLm);
  a->state = nullptr;
  a->flags = nullptr;
  a->chi2 = a->jtr = a->jtj = a->params = a->perrs = a->cov = nullptr;
  a->info = nullptr;
}

// one evaluation of np portraits at a.pext: basis rows, their spectra, the
// per-row Gram matrices, then k_gauss_step (fit: with the solver step)
int gauss_evaluate(ppf_ctx* ctx, const GaussPlan& g, const GaussFitArgs& a, int np, int fit,
                   const double2* tw) {
  return timed(ctx, PPF_K_GAUSS, [&] {
    if (a.njoin)
      hipLaunchKernelGGL(k_gauss_basis<true>, dim3(a.nchan, np), dim3(256), 0, ctx->stream, a);
    else
      hipLaunchKernelGGL(k_gauss_basis<false>, dim3(a.nchan, np), dim3(256), 0, ctx->stream, a);
    launch_rfft_rows(ctx->stream, g.logN, a.nbin, np * a.nchan * g.KT, a.rows,
                     const_cast<double2*>(a.spec), tw);
    if (a.njoin) {
      hipLaunchKernelGGL(k_gauss_gram<true>, dim3(a.nchan, np), dim3(256), 0, ctx->stream, a);
      hipLaunchKernelGGL(k_gauss_step<true>, dim3(np), dim3(256), 0, ctx->stream, a, fit);
    } else {
      hipLaunchKernelGGL(k_gauss_gram<false>, dim3(a.nchan, np), dim3(256), 0, ctx->stream, a);
      hipLaunchKernelGGL(k_gauss_step<false>, dim3(np), dim3(256), 0, ctx->stream, a, fit);
    }
  });
}

// PPF_ERR_INVALID when a join_of entry of the call is outside 0 .. njoin - 1;
// one small kernel and one read of its flag before any fit kernel reads
// join_of
int gauss_join_check(ppf_ctx* ctx, const GaussPlan& g, char* base, int64_t nrow, int njoin,
                     const int32_t* join_of) {
  int* bad = reinterpret_cast<int*>(base + g.oBad);
  int hbad = 0;
  HIPCHK(ctx, hipMemsetAsync(bad, 0, sizeof(int), ctx->stream));
  hipLaunchKernelGGL(k_gauss_join_check, dim3((unsigned)((nrow + 255) / 256)), dim3(256), 0,
                     ctx->stream, join_of, nrow, njoin, bad);
  HIPCHK(ctx, hipMemcpyAsync(&hbad, bad, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  if (hbad) return fail(ctx, PPF_ERR_INVALID, "join_of: a group outside 0..%d", njoin - 1);
  return PPF_OK;
}

int gauss_eval_impl(ppf_ctx* ctx, int32_t nport, int32_t nchan, int32_t nbin, int32_t ngauss,
                    int32_t njoin, const double* data, const double* freqs, const double* errs,
                    const double* params, const int32_t* code, const double* nu_ref,
                    const int32_t* join_of, const double* dm_coef, double* chi2, double* jtr,
                    double* jtj) {
  if (!ctx || !data || !freqs || !errs || !params || !code || !nu_ref || !chi2 || !jtr || !jtj ||
      (njoin >= 0 && (!join_of || !dm_coef)))
    return fail(ctx, PPF_ERR_INVALID, "null argument");
  if (nport <= 0) return PPF_OK;
  GaussPlan g;
  if (int r = gauss_plan(ctx, nport, nchan, nbin, ngauss, njoin, false, &g)) return r;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const double2* tw;
  if (int r = twiddles(ctx, nbin, &tw)) return r;
  if (int r = ensure(ctx, ctx->buf[kWs], g.total)) return r;
  char* base = static_cast<char*>(ctx->buf[kWs].p);
  if (njoin >= 0)
    if (int r = gauss_join_check(ctx, g, base, (int64_t)nport * nchan, njoin, join_of)) return r;
  GaussFitArgs a;
  gauss_args(g, base, nchan, nbin, ngauss, njoin, &a);
  for (int64_t p0 = 0; p0 < nport; p0 += g.chunk) {
    const int np = (int)std::min<int64_t>(g.chunk, nport - p0);
    a.freqs = freqs + (size_t)p0 * nchan;
    a.errs = errs + (size_t)p0 * nchan;
    a.code = code + (size_t)p0 * 3;
    a.nu_ref = nu_ref + p0;
    if (njoin >= 0) {
      a.join_of = join_of + (size_t)p0 * nchan;
      a.dm_coef = dm_coef + (size_t)p0 * nchan;
    }
    a.chi2 = chi2 + p0;
    a.jtr = jtr + (size_t)p0 * g.npar;
    a.jtj = jtj + (size_t)p0 * g.npar * g.npar;
    HIPCHK(ctx, hipMemcpyAsync(a.pext, params + (size_t)p0 * g.npar,
                               (size_t)np * g.npar * sizeof(double), hipMemcpyDeviceToDevice,
                               ctx->stream));
    if (int r = timed(ctx, PPF_K_GAUSS, [&] {
          launch_rfft_rows(ctx->stream, g.logN, nbin, np * nchan,
                           data + (size_t)p0 * nchan * nbin, const_cast<double2*>(a.dspec), tw);
        }))
      return r;
    if (int r = gauss_evaluate(ctx, g, a, np, 0, tw)) return r;
  }
  return PPF_OK;
}

int gauss_fit_impl(ppf_ctx* ctx, int32_t nport, int32_t nchan, int32_t nbin, int32_t ngauss,
                   int32_t njoin, const double* data, const double* freqs, const double* errs,
                   const double* init, const int32_t* flags, const int32_t* code,
                   const double* nu_ref, const int32_t* join_of, const double* dm_coef,
                   double ftol, double xtol, int32_t max_nfev, double* params,
                   double* param_errs, double* cov, double* chi2, int32_t* info) {
  if (!ctx || !data || !freqs || !errs || !init || !flags || !code || !nu_ref || !params ||
      !param_errs || !chi2 || !info || (njoin >= 0 && (!join_of || !dm_coef)))
    return fail(ctx, PPF_ERR_INVALID, "null argument");
  if (nport <= 0) return PPF_OK;
  if (!(ftol >= 0.0) || !(xtol >= 0.0) || max_nfev < 0)
    return fail(ctx, PPF_ERR_INVALID, "ftol=%g xtol=%g max_nfev=%d", ftol, xtol, max_nfev);
  GaussPlan g;
  if (int r = gauss_plan(ctx, nport, nchan, nbin, ngauss, njoin, true, &g)) return r;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const double2* tw;
  if (int r = twiddles(ctx, nbin, &tw)) return r;
  if (int r = ensure(ctx, ctx->buf[kWs], g.total)) return r;
  char* base = static_cast<char*>(ctx->buf[kWs].p);
  if (njoin >= 0)
    if (int r = gauss_join_check(ctx, g, base, (int64_t)nport * nchan, njoin, join_of)) return r;
  GaussFitArgs a;
  gauss_args(g, base, nchan, nbin, ngauss, njoin, &a);
  a.ftol = ftol;
  a.xtol = xtol;
  a.max_nfev = max_nfev;
  a.state = reinterpret_cast<GaussFitState*>(base + g.oState);
  std::vector<GaussFitState> hs((size_t)g.chunk);
  const int64_t hard_cap = max_nfev > 0 ? max_nfev : 2000 * (int64_t)(g.npar + 1);
  for (int64_t p0 = 0; p0 < nport; p0 += g.chunk) {
    const int np = (int)std::min<int64_t>(g.chunk, nport - p0);
    a.freqs = freqs + (size_t)p0 * nchan;
    a.errs = errs + (size_t)p0 * nchan;
    a.code = code + (size_t)p0 * 3;
    a.nu_ref = nu_ref + p0;
    a.flags = flags + (size_t)p0 * g.npar;
    if (njoin >= 0) {
      a.join_of = join_of + (size_t)p0 * nchan;
      a.dm_coef = dm_coef + (size_t)p0 * nchan;
    }
    a.chi2 = chi2 + p0;
    a.params = params + (size_t)p0 * g.npar;
    a.perrs = param_errs + (size_t)p0 * g.npar;
    a.cov = cov ? cov + (size_t)p0 * g.npar * g.npar : nullptr;
    a.info = info + (size_t)p0 * 4;
    HIPCHK(ctx, hipMemsetAsync(a.lm, 0, (size_t)np * kGfLmDoubles * sizeof(double), ctx->stream));
    if (int r = timed(ctx, PPF_K_GAUSS, [&] {
          launch_rfft_rows(ctx->stream, g.logN, nbin, np * nchan,
                           data + (size_t)p0 * nchan * nbin, const_cast<double2*>(a.dspec), tw);
          if (a.njoin)
            hipLaunchKernelGGL(k_gauss_init<true>, dim3(np), dim3(256), 0, ctx->stream, a,
                               init + (size_t)p0 * g.npar, a.flags);
          else
            hipLaunchKernelGGL(k_gauss_init<false>, dim3(np), dim3(256), 0, ctx->stream, a,
                               init + (size_t)p0 * g.npar, a.flags);
        }))
      return r;
    // the host reads the portraits' states once per iteration and stops when
    // every one is done (each ends by its own cap at the latest)
    for (int64_t it = 0; it <= hard_cap; ++it) {
      if (int r = gauss_evaluate(ctx, g, a, np, 1, tw)) return r;
      HIPCHK(ctx, hipMemcpyAsync(hs.data(), a.state, (size_t)np * sizeof(GaussFitState),
                                 hipMemcpyDeviceToHost, ctx->stream));
      HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
      bool all_done = true;
      for (int p = 0; p < np; ++p) all_done = all_done && hs[p].done != 0;
      if (all_done) break;
    }
  }
  return PPF_OK;
}

}  // namespace

extern "C" {

int ppf_gauss_eval(ppf_ctx* ctx, int32_t nport, int32_t nchan, int32_t nbin, int32_t ngauss,
                   const double* data, const double* freqs, const double* errs,
                   const double* params, const int32_t* code, const double* nu_ref, double* chi2,
                   double* jtr, double* jtj) {
  return gauss_eval_impl(ctx, nport, nchan, nbin, ngauss, -1, data, freqs, errs, params, code,
                         nu_ref, nullptr, nullptr, chi2, jtr, jtj);
}

int ppf_gauss_eval_join(ppf_ctx* ctx, int32_t nport, int32_t nchan, int32_t nbin, int32_t ngauss,
                        int32_t njoin, const double* data, const double* freqs,
                        const double* errs, const double* params, const int32_t* code,
                        const double* nu_ref, const int32_t* join_of, const double* dm_coef,
                        double* chi2, double* jtr, double* jtj) {
  if (njoin < 0) return fail(ctx, PPF_ERR_UNSUPPORTED, "njoin=%d: 1..%d join groups in a fit",
                             njoin, kFitMaxJoin);
  return gauss_eval_impl(ctx, nport, nchan, nbin, ngauss, njoin, data, freqs, errs, params, code,
                         nu_ref, join_of, dm_coef, chi2, jtr, jtj);
}

int ppf_gauss_fit_batch(ppf_ctx* ctx, int32_t nport, int32_t nchan, int32_t nbin, int32_t ngauss,
                        const double* data, const double* freqs, const double* errs,
                        const double* init, const int32_t* flags, const int32_t* code,
                        const double* nu_ref, double ftol, double xtol, int32_t max_nfev,
                        double* params, double* param_errs, double* cov, double* chi2,
                        int32_t* info) {
  return gauss_fit_impl(ctx, nport, nchan, nbin, ngauss, -1, data, freqs, errs, init, flags, code,
                        nu_ref, nullptr, nullptr, ftol, xtol, max_nfev, params, param_errs, cov,
                        chi2, info);
}

int ppf_gauss_fit_join_batch(ppf_ctx* ctx, int32_t nport, int32_t nchan, int32_t nbin,
                             int32_t ngauss, int32_t njoin, const double* data,
                             const double* freqs, const double* errs, const double* init,
                             const int32_t* flags, const int32_t* code, const double* nu_ref,
                             const int32_t* join_of, const double* dm_coef, double ftol,
                             double xtol, int32_t max_nfev, double* params, double* param_errs,
                             double* cov, double* chi2, int32_t* info) {
  if (njoin < 0) return fail(ctx, PPF_ERR_UNSUPPORTED, "njoin=%d: 1..%d join groups in a fit",
                             njoin, kFitMaxJoin);
  return gauss_fit_impl(ctx, nport, nchan, nbin, ngauss, njoin, data, freqs, errs, init, flags,
                        code, nu_ref, join_of, dm_coef, ftol, xtol, max_nfev, params, param_errs,
                        cov, chi2, info);
}

int ppf_gauss_bank(ppf_ctx* ctx, int32_t nprof, int32_t nbin, int32_t nwid, const double* resid,
                   const double* errs, const double* taun, const double* widths, double* s2,
                   double* best, int32_t* best_idx) {
  if (!ctx || !resid || !errs || !taun || !widths || !best || !best_idx)
    return fail(ctx, PPF_ERR_INVALID, "null argument");
  if (nprof <= 0) return PPF_OK;
  const int l = ilog2_exact(nbin);
  if (l < 6 || nbin > 8192)
    return fail(ctx, PPF_ERR_UNSUPPORTED, "nbin=%d: a power of two in [64, 8192]", nbin);
  if (nwid < 1 || nwid > kBankMaxWid)
    return fail(ctx, PPF_ERR_UNSUPPORTED, "nwid=%d: 1..%d widths in a bank", nwid, kBankMaxWid);
  GaussBankArgs a;
  for (int w = 0; w < nwid; ++w) {
    if (!(widths[w] > 0.0) || !(widths[w] <= 0.25))
      return fail(ctx, PPF_ERR_INVALID, "widths[%d]=%g: a FWHM in (0, 0.25]", w, widths[w]);
    a.widths[w] = widths[w];
  }
  for (int w = nwid; w < kBankMaxWid; ++w) a.widths[w] = 0.0;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const int logN = l - 1, NH = nbin / 2 + 1;
  if (int r = twiddles(ctx, nbin, &a.tw)) return r;
  // scratch per profile: the residual spectrum and one record per width
  const size_t bSpec = (size_t)NH * sizeof(double2), bPart = (size_t)nwid * 4 * sizeof(double);
  const int64_t chunk = std::max<int64_t>(
      1, std::min<int64_t>({(int64_t)nprof, ctx->ws_limit / (int64_t)(bSpec + bPart + 512), 65535}));
  const size_t oPart = align256((size_t)chunk * bSpec);
  if (int r = ensure(ctx, ctx->buf[kWs], oPart + (size_t)chunk * bPart)) return r;
  char* base = static_cast<char*>(ctx->buf[kWs].p);
  double2* rspec = reinterpret_cast<double2*>(base);
  a.nbin = nbin;
  a.nwid = nwid;
  a.fwhm = 2.0 * std::sqrt(2.0 * std::log(2.0));
  a.sqrt2pi = std::sqrt(2.0 * M_PI);
  a.rspec = rspec;
  a.part = reinterpret_cast<double*>(base + oPart);
  for (int64_t p0 = 0; p0 < nprof; p0 += chunk) {
    const int np = (int)std::min<int64_t>(chunk, nprof - p0);
    a.errs = errs + p0;
    a.taun = taun + p0;
    a.s2 = s2 ? s2 + (size_t)p0 * nwid * nbin : nullptr;
    a.best = best + (size_t)p0 * 4;
    a.best_idx = best_idx + (size_t)p0 * 2;
    if (int r = timed(ctx, PPF_K_GBANK, [&] {
          launch_rfft_rows(ctx->stream, logN, nbin, np, resid + (size_t)p0 * nbin, rspec, a.tw);
          LOGN_SWITCH(logN, hipLaunchKernelGGL(k_gauss_bank<LG>, dim3(nwid, np), dim3(kBlock), 0,
                                               ctx->stream, a));
          hipLaunchKernelGGL(k_gauss_bank_best, dim3((np + 63) / 64), dim3(64), 0, ctx->stream, a,
                             np);
        }))
      return r;
  }
  return PPF_OK;
}

}  // extern "C"
