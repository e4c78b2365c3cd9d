// ppfit_capi_swt.hip -- the wavelet entry points of libppfit (ppfit_swt.hip):
// smoothing at given levels and factors, their objective, and the search.
#include "ppfit_host.hpp"

namespace {

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
  std::vector<int32_t> h;
  if (int r = fetch(ctx, nlevel, (size_t)nrow, h)) return r;
  *L = 0;
  for (int r = 0; r < nrow; ++r) {
    if (int e = swt_check_level(ctx, nbin, h[r])) return e;
    *L = std::max(*L, (int)h[r]);
  }
  return PPF_OK;
}

// What the three entry points share once their arguments are checked: the
// twiddles, the workspace of a chunk of rows (L levels each) and the loop
// over the chunks.  work(a, r0, nr) makes the launches of rows r0 .. r0 + nr,
// with a holding the settings, the workspace arrays and a.rows = the chunk's
// rows; it sets the arrays of its own entry point.
template <typename F>
int swt_chunks(ppf_ctx* ctx, int nrow, int nbin, int L, int threshtype, double tol,
               const double* rows, F&& work) {
  const double2* tw;
  if (int r = twiddles(ctx, nbin, &tw)) return r;
  WsPlan ws;
  const int wW = ws.array((size_t)L * 2 * nbin * sizeof(double));
  const int wMed = ws.array((size_t)L * sizeof(double));
  const int wNz = ws.array(sizeof(int));
  const int wNoise = ws.array(sizeof(double));
  const int wGrid = ws.array((size_t)L * kSwtGrid * sizeof(double));
  const int wPf = ws.array((size_t)L * sizeof(double));
  const int wPv = ws.array((size_t)L * sizeof(double));
  // (64 + 4: the row's size was once counted 4 bytes above the arrays' sum; it
  // stays so that a workspace limit gives the chunk it always gave)
  ws.lay_out(nrow, ctx->ws_limit, 64 + 4, 65535);
  if (int r = hold_workspace(ctx, ws)) return r;
  for (int64_t r0 = 0; r0 < nrow; r0 += ws.chunk) {
    const int nr = (int)std::min<int64_t>(ws.chunk, nrow - r0);
    SwtArgs a;
    std::memset(&a, 0, sizeof(a));
    a.nbin = nbin;
    a.L = L;
    a.soft = threshtype == PPF_THRESH_SOFT;
    a.kc = noise_kc(nbin);
    a.tol = tol;
    a.sq2ln = std::sqrt(2.0 * std::log((double)nbin));
    a.tw = tw;
    a.W = ws.at<double>(wW);
    a.med = ws.at<double>(wMed);
    a.nz = ws.at<int>(wNz);
    a.noise = ws.at<double>(wNoise);
    a.fgrid = ws.at<double>(wGrid);
    a.pfact = ws.at<double>(wPf);
    a.pfun = ws.at<double>(wPv);
    a.rows = rows + (size_t)r0 * nbin;
    if (int r = work(a, r0, nr)) return r;
  }
  return PPF_OK;
}

// dynamic LDS of the transform kernels
size_t swt_lds(int nbin) { return 2 * (size_t)nbin * sizeof(double); }

// forward transform, medians (deepest: only each row's deepest level) and,
// with noise, get_noise_PS of the nr rows a.rows
void swt_launch_forward(ppf_ctx* ctx, const SwtArgs& a, int nr, int logN, int deepest, bool noise) {
  hipLaunchKernelGGL(k_swt_forward, dim3(nr), dim3(kBlock), swt_lds(a.nbin), ctx->stream, a);
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
  const size_t lds = swt_lds(nbin);
  return swt_chunks(ctx, nrow, nbin, L, threshtype, 0.0, rows, [&](SwtArgs& a, int64_t r0, int nr) {
    a.nlev = nlevel + r0;
    a.fact = fact + r0;
    a.out = out + (size_t)r0 * nbin;
    return timed(ctx, PPF_K_SWT, [&] {
      swt_launch_forward(ctx, a, nr, logN, 1, false);
      hipLaunchKernelGGL(k_swt_smooth, dim3(nr), dim3(kBlock), lds, ctx->stream, a, 0);
    });
  });
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
  const size_t lds = swt_lds(nbin);
  return swt_chunks(ctx, nrow, nbin, L, threshtype, rchi2_tol, rows,
                    [&](SwtArgs& a, int64_t r0, int nr) {
    a.nlev = nlevel + r0;
    a.fact = fact + r0;
    a.o_obj = obj + r0;
    a.o_rchi2 = red_chi2 + r0;
    return timed(ctx, PPF_K_SWT, [&] {
      swt_launch_forward(ctx, a, nr, logN, 1, true);
      SWT_SWITCH(logN, hipLaunchKernelGGL(k_swt_objective<LG>, dim3(1, 1, nr), dim3(kBlock), lds,
                                          ctx->stream, a, 1));
    });
  });
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
  const size_t lds = swt_lds(nbin);
  return swt_chunks(ctx, nrow, nbin, L, threshtype, rchi2_tol, rows,
                    [&](SwtArgs& a, int64_t r0, int nr) -> int {
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
    return PPF_OK;
  });
}

}  // extern "C"
