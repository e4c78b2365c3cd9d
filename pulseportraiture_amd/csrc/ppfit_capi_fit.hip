// ppfit_capi_fit.hip -- ppf_fit_portrait_batch and ppf_fit_portrait_batch_raw:
// workspace plan, stages, argument binding and the two launch schedules.
#include "ppfit_host.hpp"
#include "ppfits.h"  // PPFITS_RAW_*

namespace {

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

// ---------------------------------------------------------------------------
// ppf_fit_portrait_batch: workspace plan, stages, argument binding
// ---------------------------------------------------------------------------

// Workspace plan of one fit call: the arrays of a chunk of subints one after
// another in the context's workspace buffer.  Each array's per-subint size is
// written here and nowhere else.
struct FitWorkspace : WsPlan {
  int X, R, sig, dsum, st, acc, wsc, T, G;  // the arrays of a subint (WsPlan::at)

  FitWorkspace(int nchan, int NHP, bool taylor, bool wide, int64_t ws_limit, int64_t nsub) {
    const size_t bR = (size_t)NHP * sizeof(double2);
    const size_t bC = (size_t)nchan * sizeof(double);
    X = array((size_t)nchan * NHP * sizeof(double2));
    R = array(bR);
    // (a second R-sized row that no kernel uses; it stays in the plan so that a
    // workspace limit gives the chunk, and so the launches, it always gave)
    array(bR);
    sig = array(bC);
    dsum = array(bC);
    st = array(sizeof(SolveState));
    acc = array((size_t)2 * nchan * 10 * sizeof(double));
    wsc = array((size_t)nchan * 8 * sizeof(double));
    T = array(taylor ? (size_t)2 * nchan * kMT * sizeof(double) : 0);
    // per-channel tables in HBM (the WIDE kernels, ppfit_kernels.hpp chan_tables)
    G = array(wide ? align256(std::max(meta_lds(nchan), xspec_dyn_lds(nchan))) : 0);
    lay_out(nsub, ws_limit, 1024);
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
    fa.T = per[T] ? at<double>(T, sub) : nullptr;
    fa.gdyn = sa.gdyn = per[G] ? at<unsigned char>(G, sub) : nullptr;
    fa.gdyn_stride = sa.gdyn_stride = per[G];
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

// The data pass.  Generic length: every row's rfft -- the mixed-radix FFT
// where the length has one, else the DFT on the matrix cores -- into the X
// rows, then the per-subint pass (ppfit_generic.hip) (data-spectrum
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
      if (sa.spec_mode == PPF_SPEC_USE) {
        // the spectra are in the cache
      } else if (L.logN == kLogNSmooth) {
        SMOOTH_SWITCH(nbin, hipLaunchKernelGGL(k_data_fft_rows<Row>, dim3(nrows), dim3(kBlock),
                                               lds(kLdsRow), st, rows, dst, sa.NHP, sa.tw, row));
      } else if (nbin <= kGenLdsTw) {
        hipLaunchKernelGGL(k_dft_rows_mfma<true>, g, dim3(kBlock), dft_mfma_lds(nbin, true), st,
                           rows, dst, nrows, nbin, sa.NHP, sa.tw);
      } else {
        hipLaunchKernelGGL(k_dft_rows_mfma<false>, g, dim3(kBlock), dft_mfma_lds(nbin, false),
                           st, rows, dst, nrows, nbin, sa.NHP, sa.tw);
      }
      hipLaunchKernelGGL(k_data_post_gen, dim3(n), dim3(kBlock), 0, st, sa, nbin);
    }
    const dim3 g(n);
    if (sa.raw) {  // rows of 16-bit samples (ppf_fit_portrait_batch_raw)
      LOGN_SWITCH(L.logN,
                  WIDE_SWITCH(L.wide, hipLaunchKernelGGL((k_data_xspec<LG, WD, true>), g,
                                                         dim3(XspecCfg<LG>::WPB * 64),
                                                         L.lds_xspec, st, sa)));
      return;
    }
    LOGN_SWITCH(L.logN, WIDE_SWITCH(L.wide, hipLaunchKernelGGL((k_data_xspec<LG, WD, false>), g,
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
  // the fused moment pass over X stages through the same dynamic LDS first
  const bool stage = PPF_MOM_STAGE && mom && !fa.Dsp;
  const size_t lds = stage ? std::max(L.lds_taylor, kWaves * kMomStageBytes) : L.lds_taylor;
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
// *logN as check_nbin_any gives it.  raw: the data are its samples, not
// d->data.
int check_fit_desc(ppf_ctx* ctx, const ppf_fit_desc* d, const ppf_raw_subints* raw,
                   const ppf_fit_result* o, int* logN) {
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
  if (raw && d->data)
    return fail(ctx, PPF_ERR_INVALID, "a raw fit takes its data from the samples: desc->data "
                "must be NULL");
  if (raw && (!raw->raw || !raw->scl || !raw->offs))
    return fail(ctx, PPF_ERR_INVALID, "missing required input pointer");
  if ((!raw && !d->data) || !d->model || !d->freqs || !d->P || !d->init || !d->nu_fit || !d->nu_out)
    return fail(ctx, PPF_ERR_INVALID, "missing required input pointer");
  if (!o->params || !o->param_errs || !o->nu_out || !o->cov || !o->scales || !o->scale_errs ||
      !o->channel_snrs || !o->chi2 || !o->red_chi2 || !o->snr || !o->nfev || !o->status)
    return fail(ctx, PPF_ERR_INVALID, "missing required output pointer");
  if (d->guess && d->guess_Ns < 2) return fail(ctx, PPF_ERR_INVALID, "guess_Ns must be >= 2");
  // nbin not a power of two: the generic-length data pass and template
  // spectra (ppfit_generic.hip); every solver kernel takes any nbin
  if (int r = check_nbin_any(ctx, d->nbin, logN)) return r;
  if (raw) {
    // the raw rows exist for the power-of-two data pass and 16-bit samples
    if (*logN < 0)
      return fail(ctx, PPF_ERR_UNSUPPORTED, "raw samples: nbin=%d is not a power of two in "
                  "[64, 8192] (unpack and fit the values)", d->nbin);
    if (raw->raw_type != PPFITS_RAW_I16)
      return fail(ctx, PPF_ERR_UNSUPPORTED, "raw samples: raw_type %d, only 16-bit samples "
                  "(PPFITS_RAW_I16) are read in the fit", raw->raw_type);
    if (raw->npol < 1 || raw->pmode < 0 || raw->pmode > 2 || raw->ipol < 0 ||
        raw->ipol >= raw->npol || (raw->pmode == 1 && raw->npol < 2))
      return fail(ctx, PPF_ERR_INVALID, "raw samples: pmode %d, ipol %d with npol %d",
                  raw->pmode, raw->ipol, raw->npol);
    if (reinterpret_cast<uintptr_t>(raw->raw) % 16)
      return fail(ctx, PPF_ERR_INVALID, "raw samples must be 16-byte aligned");
  }
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
void bind_fit_args(const ppf_ctx* ctx, const ppf_fit_desc* d, const ppf_raw_subints* raw,
                   const ppf_fit_result* o, SpecArgs& sa, FitArgs& fa) {
  const int nbin = d->nbin;
  sa.nchan = fa.nchan = d->nchan;
  sa.NHP = fa.NHP = nharm_pad(nbin);
  sa.kc = fa.kc = noise_kc(nbin);
  sa.guess = fa.guess = d->guess;
  sa.data = d->data;
  if (raw) {
    sa.raw = static_cast<const uint32_t*>(raw->raw);
    sa.scl = raw->scl;
    sa.offs = raw->offs;
    sa.rnpol = raw->npol;
    sa.rp0 = raw->pmode == 0 ? raw->ipol : 0;
    sa.rsum = raw->pmode == 1 ? 1 : 0;
    sa.rp1 = sa.rsum ? 1 : sa.rp0;
  }
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

// The fit call of both entry points; raw NULL: the data are d->data.
int fit_portrait_batch(ppf_ctx* ctx, const ppf_fit_desc* d, const ppf_raw_subints* raw,
                       const ppf_fit_result* o) {
  if (d->nsub <= 0) return PPF_OK;
  FitLaunch L;
  if (int r = check_fit_desc(ctx, d, raw, o, &L.logN)) return r;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const int nchan = d->nchan, nbin = d->nbin, NH = nbin / 2 + 1;
  const bool tnc = fit_is_tnc(d), ncg = d->method == PPF_METHOD_NEWTON_CG;
  const bool exact = fit_is_exact(d), taylor = fit_is_taylor(d);
  SpecArgs sa{};
  FitArgs fa{};
  bind_fit_args(ctx, d, raw, o, sa, fa);
  if (int r = fit_tables(ctx, d, sa, fa)) return r;

  // per-channel tables in HBM (the WIDE kernels, ppfit_kernels.hpp chan_tables)
  const bool wide = nchan > PPF_LDS_NCHAN || ctx->opt[PPF_OPT_HBM_TABLES] != 0;
  FitWorkspace ws(nchan, fa.NHP, taylor, wide, ctx->ws_limit, d->nsub);
  if (int r = hold_workspace(ctx, ws)) return r;
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

}  // namespace

extern "C" {

// ---------------------------------------------------------------------------
int ppf_fit_portrait_batch(ppf_ctx* ctx, const ppf_fit_desc* d, const ppf_fit_result* o) {
  if (!ctx || !d || !o) return fail(ctx, PPF_ERR_INVALID, "null argument");
  return fit_portrait_batch(ctx, d, nullptr, o);
}

int ppf_fit_portrait_batch_raw(ppf_ctx* ctx, const ppf_fit_desc* d, const ppf_raw_subints* raw,
                               const ppf_fit_result* o) {
  if (!ctx || !d || !raw || !o) return fail(ctx, PPF_ERR_INVALID, "null argument");
  return fit_portrait_batch(ctx, d, raw, o);
}

}  // extern "C"
