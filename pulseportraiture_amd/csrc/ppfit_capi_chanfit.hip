// ppfit_capi_chanfit.hip -- the entry points of the fits across channels
// (ppfit_chanfit.hip): one launch each, no workspace.
#include "ppfit_host.hpp"

namespace {

constexpr int kChanfitMaxN = 16384;

int check_chanfit_shape(ppf_ctx* ctx, int32_t nrow, int32_t n) {
  if (nrow < 1) return fail(ctx, PPF_ERR_INVALID, "nrow=%d: at least one row", nrow);
  if (n < 1 || n > kChanfitMaxN)
    return fail(ctx, PPF_ERR_INVALID, "n=%d: outside [1, %d]", n, kChanfitMaxN);
  return PPF_OK;
}

}  // namespace

extern "C" {

int ppf_powlaw_fit_rows(ppf_ctx* ctx, int32_t nrow, int32_t n, const double* y,
                        const double* errs, const double* freqs, const double* nu_ref,
                        const double* init, double ftol, double xtol, int32_t max_nfev,
                        double* out, int32_t* info) {
  if (!ctx || !y || !errs || !freqs || !nu_ref || !init || !out || !info)
    return fail(ctx, PPF_ERR_INVALID, "null argument");
  if (int r = check_chanfit_shape(ctx, nrow, n)) return r;
  if (!(ftol >= 0.0) || !(xtol >= 0.0) || max_nfev < 0)
    return fail(ctx, PPF_ERR_INVALID, "ftol=%g xtol=%g max_nfev=%d", ftol, xtol, max_nfev);
  HIPCHK(ctx, hipSetDevice(ctx->device));
  PowlawArgs a;
  a.nrow = nrow;
  a.n = n;
  a.cap = max_nfev > 0 ? max_nfev : 2000 * 3;  // leastsq: 2000 (npar + 1)
  a.ftol = ftol;
  a.xtol = xtol;
  a.y = y;
  a.errs = errs;
  a.freqs = freqs;
  a.nu_ref = nu_ref;
  a.init = init;
  a.out = out;
  a.info = info;
  // 64 points per register slot; above 512 the row stays in memory
  const int nj = n <= 64 ? 1 : n <= 128 ? 2 : n <= 256 ? 4 : n <= 512 ? 8 : 0;
  const dim3 g((unsigned)(((int64_t)nrow + kWaves - 1) / kWaves)), b(kBlock);
  return timed(ctx, PPF_K_GAUSS, [&] {
    switch (nj) {
      case 1: hipLaunchKernelGGL(k_powlaw_fit<1>, g, b, 0, ctx->stream, a); break;
      case 2: hipLaunchKernelGGL(k_powlaw_fit<2>, g, b, 0, ctx->stream, a); break;
      case 4: hipLaunchKernelGGL(k_powlaw_fit<4>, g, b, 0, ctx->stream, a); break;
      case 8: hipLaunchKernelGGL(k_powlaw_fit<8>, g, b, 0, ctx->stream, a); break;
      default: hipLaunchKernelGGL(k_powlaw_fit<0>, g, b, 0, ctx->stream, a); break;
    }
  });
}

int ppf_line_fit_rows(ppf_ctx* ctx, int32_t nrow, int32_t n, const double* x, const double* y,
                      const double* w, double* out) {
  if (!ctx || !x || !y || !w || !out) return fail(ctx, PPF_ERR_INVALID, "null argument");
  if (int r = check_chanfit_shape(ctx, nrow, n)) return r;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const dim3 g((unsigned)(((int64_t)nrow + kWaves - 1) / kWaves)), b(kBlock);
  return timed(ctx, PPF_K_GAUSS, [&] {
    hipLaunchKernelGGL(k_line_fit, g, b, 0, ctx->stream, (int)nrow, (int)n, x, y, w, out);
  });
}

}  // extern "C"
