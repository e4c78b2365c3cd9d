// ppfit_capi_gauss.hip -- the Gaussian-component entry points of libppfit:
// evaluations and fits of portraits (ppfit_gauss.hip), alone or joined over
// receivers, and the matched-filter bank (ppfit_gbank.hip).
#include "ppfit_host.hpp"

namespace {

// Shapes of a Gaussian-component fit and the workspace of a chunk of
// portraits (ppfit_gauss.hip).
struct GaussPlan {
  int npar, KT, KB, npairs, NH, logN;
  WsPlan ws;
  int wRows, wSpec, wDspec, wCoef, wTaun, wGram, wPext, wLm, wState;  // a portrait's arrays
  size_t oBad;  // the flag of k_gauss_join_check, behind them
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
  WsPlan& ws = g->ws;
  g->wRows = ws.array(rows * g->KT * nbin * sizeof(double));
  g->wSpec = ws.array(rows * g->KT * g->NH * sizeof(double2));
  g->wDspec = ws.array(rows * g->NH * sizeof(double2));
  g->wCoef = ws.array(rows * g->npar * sizeof(double));
  g->wTaun = ws.array(rows * sizeof(double));
  g->wGram = ws.array(rows * g->npairs * sizeof(double));
  g->wPext = ws.array((size_t)g->npar * sizeof(double));
  g->wLm = ws.array(fit ? (size_t)kGfLmDoubles * sizeof(double) : 0);
  g->wState = ws.array(sizeof(GaussFitState));
  ws.lay_out(nport, ctx->ws_limit, 4096, 65535);
  g->oBad = ws.total;
  if (join) ws.total += 256;
  return PPF_OK;
}

void gauss_args(const GaussPlan& g, int nchan, int nbin, int ngauss, int njoin, GaussFitArgs* a) {
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
  a->rows = g.ws.at<double>(g.wRows);
  a->spec = g.ws.at<double2>(g.wSpec);
  a->dspec = g.ws.at<double2>(g.wDspec);
  a->coef = g.ws.at<double>(g.wCoef);
  a->taun = g.ws.at<double>(g.wTaun);
  a->gram = g.ws.at<double>(g.wGram);
  a->pext = g.ws.at<double>(g.wPext);
  a->lm = g.ws.at<double>(g.wLm);
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
    JOIN_SWITCH(a.njoin, {
      hipLaunchKernelGGL(k_gauss_basis<JN>, dim3(a.nchan, np), dim3(256), 0, ctx->stream, a);
      launch_rfft_rows(ctx->stream, g.logN, a.nbin, np * a.nchan * g.KT, a.rows,
                       const_cast<double2*>(a.spec), tw);
      hipLaunchKernelGGL(k_gauss_gram<JN>, dim3(a.nchan, np), dim3(256), 0, ctx->stream, a);
      hipLaunchKernelGGL(k_gauss_step<JN>, dim3(np), dim3(256), 0, ctx->stream, a, fit);
    });
  });
}

// PPF_ERR_INVALID when a join_of entry of the call is outside 0 .. njoin - 1;
// one small kernel and one read of its flag before any fit kernel reads
// join_of
int gauss_join_check(ppf_ctx* ctx, const GaussPlan& g, int64_t nrow, int njoin,
                     const int32_t* join_of) {
  int* bad = reinterpret_cast<int*>(g.ws.base + g.oBad);
  int hbad = 0;
  HIPCHK(ctx, hipMemsetAsync(bad, 0, sizeof(int), ctx->stream));
  hipLaunchKernelGGL(k_gauss_join_check, dim3((unsigned)((nrow + 255) / 256)), dim3(256), 0,
                     ctx->stream, join_of, nrow, njoin, bad);
  HIPCHK(ctx, hipMemcpyAsync(&hbad, bad, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  if (hbad) return fail(ctx, PPF_ERR_INVALID, "join_of: a group outside 0..%d", njoin - 1);
  return PPF_OK;
}

// What an evaluation and a fit do between their own argument checks and
// their loop over the chunks: the plan, the device, twiddles, the workspace,
// the join check, and the arguments that no chunk changes.
int gauss_begin(ppf_ctx* ctx, int nport, int nchan, int nbin, int ngauss, int njoin, bool fit,
                const int32_t* join_of, GaussPlan* g, const double2** tw, GaussFitArgs* a) {
  if (int r = gauss_plan(ctx, nport, nchan, nbin, ngauss, njoin, fit, g)) return r;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  if (int r = twiddles(ctx, nbin, tw)) return r;
  if (int r = hold_workspace(ctx, g->ws)) return r;
  if (njoin >= 0)
    if (int r = gauss_join_check(ctx, *g, (int64_t)nport * nchan, njoin, join_of)) return r;
  gauss_args(*g, nchan, nbin, ngauss, njoin, a);
  return PPF_OK;
}

// the caller's per-portrait arrays that both take, from portrait p0 on
// (join_of and dm_coef: null without a join)
void gauss_slice(GaussFitArgs& a, int64_t p0, int nchan, const double* freqs, const double* errs,
                 const int32_t* code, const double* nu_ref, const int32_t* join_of,
                 const double* dm_coef, double* chi2) {
  a.freqs = freqs + (size_t)p0 * nchan;
  a.errs = errs + (size_t)p0 * nchan;
  a.code = code + (size_t)p0 * 3;
  a.nu_ref = nu_ref + p0;
  a.join_of = join_of ? join_of + (size_t)p0 * nchan : nullptr;
  a.dm_coef = dm_coef ? dm_coef + (size_t)p0 * nchan : nullptr;
  a.chi2 = chi2 + p0;
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
  const double2* tw;
  GaussFitArgs a;
  if (int r = gauss_begin(ctx, nport, nchan, nbin, ngauss, njoin, false, join_of, &g, &tw, &a))
    return r;
  for (int64_t p0 = 0; p0 < nport; p0 += g.ws.chunk) {
    const int np = (int)std::min<int64_t>(g.ws.chunk, nport - p0);
    gauss_slice(a, p0, nchan, freqs, errs, code, nu_ref, join_of, dm_coef, chi2);
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
  const double2* tw;
  GaussFitArgs a;
  if (int r = gauss_begin(ctx, nport, nchan, nbin, ngauss, njoin, true, join_of, &g, &tw, &a))
    return r;
  a.ftol = ftol;
  a.xtol = xtol;
  a.max_nfev = max_nfev;
  a.state = g.ws.at<GaussFitState>(g.wState);
  std::vector<GaussFitState> hs;
  const int64_t hard_cap = max_nfev > 0 ? max_nfev : 2000 * (int64_t)(g.npar + 1);
  for (int64_t p0 = 0; p0 < nport; p0 += g.ws.chunk) {
    const int np = (int)std::min<int64_t>(g.ws.chunk, nport - p0);
    gauss_slice(a, p0, nchan, freqs, errs, code, nu_ref, join_of, dm_coef, chi2);
    a.flags = flags + (size_t)p0 * g.npar;
    a.params = params + (size_t)p0 * g.npar;
    a.perrs = param_errs + (size_t)p0 * g.npar;
    a.cov = cov ? cov + (size_t)p0 * g.npar * g.npar : nullptr;
    a.info = info + (size_t)p0 * 4;
    HIPCHK(ctx, hipMemsetAsync(a.lm, 0, (size_t)np * kGfLmDoubles * sizeof(double), ctx->stream));
    if (int r = timed(ctx, PPF_K_GAUSS, [&] {
          launch_rfft_rows(ctx->stream, g.logN, nbin, np * nchan,
                           data + (size_t)p0 * nchan * nbin, const_cast<double2*>(a.dspec), tw);
          JOIN_SWITCH(a.njoin, hipLaunchKernelGGL(k_gauss_init<JN>, dim3(np), dim3(256), 0,
                                                  ctx->stream, a, init + (size_t)p0 * g.npar,
                                                  a.flags));
        }))
      return r;
    // the host reads the portraits' states once per iteration and stops when
    // every one is done (each ends by its own cap at the latest)
    for (int64_t it = 0; it <= hard_cap; ++it) {
      if (int r = gauss_evaluate(ctx, g, a, np, 1, tw)) return r;
      bool all_done;
      if (int r = poll_done(ctx, a.state, np, hs, &all_done)) return r;
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
  WsPlan ws;
  const int wSpec = ws.array((size_t)NH * sizeof(double2));
  const int wPart = ws.array((size_t)nwid * 4 * sizeof(double));
  ws.lay_out(nprof, ctx->ws_limit, 512, 65535);
  if (int r = hold_workspace(ctx, ws)) return r;
  const int64_t chunk = ws.chunk;
  double2* rspec = ws.at<double2>(wSpec);
  a.nbin = nbin;
  a.nwid = nwid;
  a.fwhm = 2.0 * std::sqrt(2.0 * std::log(2.0));
  a.sqrt2pi = std::sqrt(2.0 * M_PI);
  a.rspec = rspec;
  a.part = ws.at<double>(wPart);
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
