// ppfit_capi_rows.hip -- the row, archive and template entry points of
// libppfit: one or a few launches over rows of nbin each.
#include "ppfit_host.hpp"

namespace {

// Number of template rows = 1 + max(model_idx) (device array or null: one
// row); the caller sizes model.  A negative index is an error.
int count_model_rows(ppf_ctx* ctx, const int32_t* model_idx, int32_t nprof, int* nmodel) {
  *nmodel = 1;
  if (!model_idx) return PPF_OK;
  std::vector<int32_t> h;
  if (int r = fetch(ctx, model_idx, (size_t)nprof, h)) return r;
  for (int32_t v : h) {
    if (v < 0) return fail(ctx, PPF_ERR_INVALID, "negative model_idx");
    *nmodel = std::max(*nmodel, (int)v + 1);
  }
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

// What ppf_scrunch_subints adds to ppf_rotate_fscrunch's sum: the weights and
// phases [nsub][ngroup nchan] to lay out per unit, 16-bit rows in place of
// fp64 ones, and the division by W with the mean of b adjacent bins.
struct ScrunchExtra {
  const FsRaw* raw;       // null: fp64 rows
  const double* weights;
  const double* phase;
  int npo, ngroup, b;
  double* wout;           // [nsub][ngroup]
};

// prof[u] = irfft(sum_n weight[u][n] rfft(row(u, n)) e^{2 pi i k phase[u][n]}) for
// nunit units of nchan channels; with sx, phase and weight come from it and
// prof [nunit][nbin / b] is the scrunched profile.
int fscrunch_units(ppf_ctx* ctx, int64_t nunit, int nchan, int nbin, int logN,
                   const double* data, const double* phase, const double* weight, double* prof,
                   const ScrunchExtra* sx) {
  const double2* tw;
  if (int r = twiddles(ctx, nbin, &tw)) return r;
  const int NH = nbin / 2 + 1;
  // slices of kFsSlice channels whatever the call holds: a unit's profile
  // is summed in the same order alone or among others
  const int nslice = (nchan + kFsSlice - 1) / kFsSlice;
  // per unit: the slices' partial spectra, then the unit's spectrum; units in
  // chunks under the workspace limit (and one launch's grid)
  WsPlan ws;
  const int wPart = ws.array((size_t)nslice * NH * sizeof(double2));
  const int wSpec = ws.array((size_t)NH * sizeof(double2));
  // scrunch: the unit's weights and phases, W, and its profile at nbin bins
  const int wWx = sx ? ws.array((size_t)nchan * sizeof(double)) : -1;
  const int wPhx = sx ? ws.array((size_t)nchan * sizeof(double)) : -1;
  const int wW = sx ? ws.array(sizeof(double)) : -1;
  const int wProf = sx ? ws.array((size_t)nbin * sizeof(double)) : -1;
  // slack: 256 bytes of alignment per array
  ws.lay_out(nunit, ctx->ws_limit, sx ? 1536 : 512, (int64_t)0x7fffffff / nslice);
  if (int r = hold_workspace(ctx, ws)) return r;
  const int64_t chunk = ws.chunk;
  double2* partial = ws.at<double2>(wPart);
  double2* spec = ws.at<double2>(wSpec);
  const int nyq = (nbin & 1) ? -1 : nbin / 2;
  const bool wave = logN == 10;  // nbin 2048: the register FFT (2.6x the LDS kernel)
  const int nbo = sx ? nbin / sx->b : nbin;
  for (int64_t u0 = 0; u0 < nunit; u0 += chunk) {
    const int nu = (int)std::min<int64_t>(chunk, nunit - u0);
    const double* d = data ? data + (size_t)u0 * nchan * nbin : nullptr;
    const double* ph = phase ? phase + (size_t)u0 * nchan : nullptr;
    const double* w = weight ? weight + (size_t)u0 * nchan : nullptr;
    double* rows = sx ? ws.at<double>(wProf) : prof + (size_t)u0 * nbin;  // the irfft's output
    if (sx) {
      double* wx = ws.at<double>(wWx);
      double* phx = ws.at<double>(wPhx);
      if (int r = timed(ctx, PPF_K_FSCRUNCH, [&] {
            hipLaunchKernelGGL(k_scrunch_meta, dim3((unsigned)((nu + 255) / 256)), dim3(256), 0,
                               ctx->stream, sx->weights, sx->phase, u0, nu, sx->npo, sx->ngroup,
                               nchan, wx, phx, ws.at<double>(wW), sx->wout);
          }))
        return r;
      ph = phx;
      w = wx;
    }
    const unsigned grid = (unsigned)nu * (unsigned)nslice;
    const size_t count = (size_t)nu * NH;
    if (sx && sx->raw) {  // 16-bit rows: the power-of-two kernels' raw twins
      FsRaw fr = *sx->raw;
      fr.unit0 = u0;
      if (int r = timed(ctx, PPF_K_FSCRUNCH, [&] {
            if (wave)
              hipLaunchKernelGGL(k_fscrunch_w_raw, dim3(grid), dim3(256), 0, ctx->stream, fr, ph,
                                 w, partial, nchan, nslice, tw);
            else
              LOGN_SWITCH(logN, hipLaunchKernelGGL(k_fscrunch_raw<LG>, dim3(grid), dim3(kBlock),
                                                   0, ctx->stream, fr, ph, w, partial, nchan,
                                                   nslice, tw));
          }))
        return r;
    } else if (int r = timed(ctx, PPF_K_FSCRUNCH, [&] {
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
          launch_irfft_rows(ctx->stream, logN, nbin, nu, spec, rows, tw);
        }))
      return r;
    if (sx) {
      const size_t nout = (size_t)nu * nbo;
      if (int r = timed(ctx, PPF_K_FSCRUNCH, [&] {
            hipLaunchKernelGGL(k_scrunch_mean, dim3((unsigned)((nout + 255) / 256)), dim3(256), 0,
                               ctx->stream, rows, ws.at<double>(wW), prof + (size_t)u0 * nbo, nbin,
                               sx->b, nout);
          }))
        return r;
    }
  }
  return PPF_OK;
}

}  // namespace

extern "C" {

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
  WsPlan ws;
  const int wD = ws.array(brow);
  ws.lay_out(nprof, ctx->ws_limit, 0);
  if (int r = hold_workspace(ctx, ws)) return r;
  const int64_t chunk = ws.chunk;
  double2* D = ws.at<double2>(wD);
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
  RowPlan rp;
  if (int r = check_nbin_any(ctx, nbin, &rp.logN)) return r;
  if (int r = row_device(ctx, nbin, &rp)) return r;
  return timed(ctx, PPF_K_ROTATE, [&] {
    launch_rotate_rows(ctx->stream, rp.logN, nbin, nrow, in, phase, nullptr, out, rp.tw);
  });
}

int ppf_scatter_rotate_rows(ppf_ctx* ctx, int32_t nrow, int32_t nbin, const double* in,
                            const double* phase, const double* tau, double* out) {
  if (!ctx || !in || !out) return fail(ctx, PPF_ERR_INVALID, "null argument");
  if (nrow <= 0) return PPF_OK;
  RowPlan rp;
  if (int r = check_nbin_any(ctx, nbin, &rp.logN)) return r;
  if (int r = row_device(ctx, nbin, &rp)) return r;
  if (!phase) return fail(ctx, PPF_ERR_INVALID, "phase must be given (zeros for none)");
  return timed(ctx, PPF_K_ROTATE, [&] {
    launch_rotate_rows(ctx->stream, rp.logN, nbin, nrow, in, phase, tau, out, rp.tw);
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
  RowPlan rp;
  if (int r = check_nbin_any(ctx, nbin, &rp.logN)) return r;
  if (int r = row_device(ctx, nbin, &rp)) return r;
  const double2* sp = reinterpret_cast<const double2*>(spec);
  return timed(ctx, PPF_K_IRFFT, [&] {
    launch_irfft_rows(ctx->stream, rp.logN, nbin, nrow, sp, out, rp.tw);
  });
}

int ppf_noise_rows_frac(ppf_ctx* ctx, int32_t nrow, int32_t nbin, double frac, const double* in,
                        double* out) {
  if (!ctx || !in || !out) return fail(ctx, PPF_ERR_INVALID, "null argument");
  if (nrow <= 0) return PPF_OK;
  RowPlan rp;
  if (int r = check_nbin_any(ctx, nbin, &rp.logN)) return r;
  if (!(frac > 1.0) || !std::isfinite(frac))
    return fail(ctx, PPF_ERR_INVALID, "frac=%g: must be > 1 and finite", frac);
  if (int r = row_device(ctx, nbin, &rp)) return r;
  // pplib.py:2245, kc = int((1 - frac**-1) * len(pows)); frac = 4 is noise_kc
  const int kc = (int)((1.0 - 1.0 / frac) * (double)(nbin / 2 + 1));
  return timed(ctx, PPF_K_NOISE, [&] {
    ROW_SWITCH(rp.logN, nbin, hipLaunchKernelGGL(k_noise_rows<Row>, dim3(nrow), dim3(kBlock),
                                                 lds(kLdsRow), ctx->stream, in, out, kc, rp.tw,
                                                 row));
  });
}

int ppf_noise_rows(ppf_ctx* ctx, int32_t nrow, int32_t nbin, const double* in, double* out) {
  return ppf_noise_rows_frac(ctx, nrow, nbin, 4.0, in, out);
}

int ppf_noise_fit_rows(ppf_ctx* ctx, int32_t nrow, int32_t nbin, const double* in, double fact,
                       double* noise_out, int32_t* kc_out, int32_t* idx_out) {
  if (!ctx || !in || !noise_out) return fail(ctx, PPF_ERR_INVALID, "null argument");
  if (nrow <= 0) return PPF_OK;
  RowPlan rp;
  if (int r = check_nbin_any(ctx, nbin, &rp.logN)) return r;
  if (!(fact > 0.0) || !std::isfinite(fact))
    return fail(ctx, PPF_ERR_INVALID, "fact=%g: must be positive and finite", fact);
  if (int r = row_device(ctx, nbin, &rp)) return r;
  return timed(ctx, PPF_K_NOISE, [&] {
    ROW_SWITCH(rp.logN, nbin, hipLaunchKernelGGL(k_noise_fit_rows<Row>, dim3(nrow), dim3(kBlock),
                                                 lds(kLdsSpec), ctx->stream, in, fact, noise_out,
                                                 kc_out, idx_out, rp.tw, row));
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
  RowPlan rp;
  if (int r = check_nbin_any(ctx, nbin, &rp.logN)) return r;
  if (int r = row_device(ctx, nbin, &rp)) return r;
  const int NH = nbin / 2 + 1;
  // one workgroup per (slice, channel), about 2048 of them (8 per CU); nbin
  // 2048: four waves each streaming every fourth row of the slice (register
  // FFT), so a slice should hold a few groups of four
  const bool wave = rp.logN == 10;
  int nsplit = (2048 + nchan - 1) / nchan;
  if (wave && nsplit > (nsub + 3) / 4) nsplit = (nsub + 3) / 4;
  if (nsplit > nsub) nsplit = nsub;
  if (nsplit < 1) nsplit = 1;
  const size_t count = (size_t)nchan * NH;
  if (int r = ensure(ctx, ctx->buf[kAux], (size_t)nsplit * count * sizeof(double2))) return r;
  double2* partial = reinterpret_cast<double2*>(ctx->buf[kAux].p);
  if (int r = timed(ctx, PPF_K_ROT_ACCUM, [&] {
        if (wave)
          hipLaunchKernelGGL(k_rot_accum_w, dim3(nsplit * nchan), dim3(256), 0, ctx->stream, data,
                             phase, weight, partial, nsub, nchan, nsplit, rp.tw);
        else
          ROW_SWITCH(rp.logN, nbin, hipLaunchKernelGGL(k_rot_accum<Row>, dim3(nsplit * nchan),
                                                       dim3(kBlock), lds(kLdsRow), ctx->stream,
                                                       data, phase, weight, partial, nsub, nchan,
                                                       nsplit, rp.tw, row));
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

int ppf_row_transform(const ppf_ctx* ctx, int32_t nbin, int32_t* kind) {
  if (!kind) return PPF_ERR_INVALID;
  if (nbin < 16 || nbin > 8192) return PPF_ERR_UNSUPPORTED;
  static_assert(kRowPow2 == PPF_ROW_POW2 && kRowSmooth == PPF_ROW_SMOOTH &&
                kRowDirect == PPF_ROW_DIRECT, "ppfit.h names row_kind's values");
  *kind = row_kind(nbin, ctx ? ctx->opt[PPF_OPT_ROW_FFT] != 0 : true);
  return PPF_OK;
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
  return fscrunch_units(ctx, nunit, nchan, nbin, logN, data, phase, weight, prof, nullptr);
}

int ppf_scrunch_subints(ppf_ctx* ctx, int32_t nsub, int32_t npol, int32_t nchan, int32_t nbin,
                        const double* data, const ppf_raw_subints* raw, const double* weights,
                        const double* phase, int32_t f, int32_t b, double* out, double* wout) {
  if (!ctx || !weights || !phase || !out || !wout || (data == nullptr) == (raw == nullptr))
    return fail(ctx, PPF_ERR_INVALID, "null argument (data or raw, not both)");
  if (raw && (!raw->raw || !raw->scl || !raw->offs))
    return fail(ctx, PPF_ERR_INVALID, "null argument");
  if (nsub <= 0) return PPF_OK;
  if (npol <= 0 || nchan <= 0 || nbin <= 0)
    return fail(ctx, PPF_ERR_INVALID, "bad shape (%d, %d, %d)", npol, nchan, nbin);
  if (f < 1 || nchan % f) return fail(ctx, PPF_ERR_INVALID, "f=%d does not divide nchan=%d", f, nchan);
  if (b < 1 || nbin % b) return fail(ctx, PPF_ERR_INVALID, "b=%d does not divide nbin=%d", b, nbin);
  if (nbin / b < 16)
    return fail(ctx, PPF_ERR_UNSUPPORTED, "nbin / b = %d: fewer than 16 bins", nbin / b);
  int logN;
  if (int r = check_nbin_any(ctx, nbin, &logN)) return r;
  const int ngroup = nchan / f;
  if ((int64_t)nsub * npol * ngroup > 0x7fffffffLL)
    return fail(ctx, PPF_ERR_INVALID, "%lld profiles in one call", (long long)nsub * npol * ngroup);
  FsRaw fr{};
  if (raw) {
    if (raw->raw_type != PPFITS_RAW_I16 || logN < 5)
      return fail(ctx, PPF_ERR_UNSUPPORTED,
                  "raw rows: 16-bit samples at a power-of-two nbin in [64, 8192] (unpack first)");
    const bool all = raw->pmode == 0 && raw->ipol < 0;
    if (raw->npol <= 0 || raw->pmode < 0 || raw->pmode > 2 || (raw->pmode == 1 && raw->npol < 2) ||
        (raw->pmode == 0 && raw->ipol >= raw->npol) || npol != (all ? raw->npol : 1))
      return fail(ctx, PPF_ERR_INVALID, "pmode %d, ipol %d with %d stored and %d kept polarisations",
                  raw->pmode, raw->ipol, raw->npol, npol);
    if (reinterpret_cast<uintptr_t>(raw->raw) % 4)  // rows are read as packed pairs
      return fail(ctx, PPF_ERR_INVALID, "raw is not 4-byte aligned");
    fr.raw = static_cast<const uint32_t*>(raw->raw);
    fr.scl = raw->scl;
    fr.offs = raw->offs;
    fr.rnpol = raw->npol;
    fr.rsum = raw->pmode == 1;
    fr.rp0 = raw->pmode == 0 ? (all ? -1 : raw->ipol) : 0;
    fr.rp1 = fr.rsum ? 1 : fr.rp0;
    fr.npo = npol;
    fr.ngroup = ngroup;
    fr.nchan_all = nchan;
  }
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const ScrunchExtra sx{raw ? &fr : nullptr, weights, phase, npol, ngroup, b, wout};
  return fscrunch_units(ctx, (int64_t)nsub * npol * ngroup, f, nbin, logN, data, nullptr, nullptr,
                        out, &sx);
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
  RowPlan rp;
  if (int r = check_nbin_any(ctx, nbin, &rp.logN)) return r;
  if (int r = row_device(ctx, nbin, &rp)) return r;
  ResidArgs ra{data, phase, model, model_row, scale, tau, errs, dof, out};
  return timed(ctx, PPF_K_RESID, [&] {
    ROW_SWITCH(rp.logN, nbin, hipLaunchKernelGGL(k_resid_chi2<Row>, dim3(nrow), dim3(kBlock),
                                                 lds(kLdsRowInv), ctx->stream, ra, rp.tw, row));
  });
}

}  // extern "C"
