// ppfit_chanfit.hip -- fits across the channels of a row (gfx950).
//
// k_powlaw_fit: pplib.fit_powlaw (pplib.py:1763-1802) per row, the weighted
// power law y = A (nu / nu_ref)^alpha with the residual (y - model) / errs of
// fit_powlaw_function (pplib.py:1204-1217); lmfit's leastsq there, here a
// Levenberg-Marquardt under the rules of k_gauss_step (ppfit_gauss.hip):
// MINPACK's column scaling D (running maximum of the column norms), the step
// from (J^T J + lambda D^2) d = -J^T r, acceptance by the gain ratio,
// MINPACK's ftol / xtol tests.  No bounds.
//
// k_line_fit: np.polyfit(x, y, 1, w=w, cov=True) per row in closed form, as
// pplib.fit_DM_to_freq_resids calls it (pplib.py:1804-1840).
//
// One row per wave, four rows per workgroup, a row's points strided over the
// 64 lanes: lane l owns the points l + 64 j.  Every sum is a lane's partial
// in j order, then one wave_sum; no LDS, no barrier, no atomics, so a row's
// result is bitwise independent of what shares the call.  The whole fit of a
// row runs inside the launch on wave-uniform scalars, every lane the same
// control flow.
//
// The power law is exp(alpha ln(nu / nu_ref)) in fp64.  Up to 512 points a
// lane keeps ln(nu / nu_ref), y and 1 / errs of its points in registers (NJ
// slots of 64 points); above that (NJ = 0) the row is read again, and the
// logarithm taken again, in every evaluation.  A point whose errs is <= 0,
// NaN or infinite is left out (weight 0).
#include "ppfit_kernels.hpp"

namespace ppf {

namespace {

// one evaluation: chi2 = |r|^2, g = J^T r, H = J^T J with J = dr / d(A, alpha)
struct PlSums {
  double chi2, g0, g1, h00, h01, h11;
};

template <int NJ>
struct PlRow {
  double L[NJ > 0 ? NJ : 1], y[NJ > 0 ? NJ : 1], w[NJ > 0 ? NJ : 1];
  const double* yp;
  const double* ep;
  const double* fp;
  double nu_ref;
  int n;
};

__device__ __forceinline__ bool cf_usable(double e) { return e > 0.0 && isfinite(e); }

// point i of a row as (ln(nu / nu_ref), y, 1 / errs); zeros when left out
__device__ __forceinline__ void pl_point(const double* yp, const double* ep, const double* fp,
                                         int i, double nu_ref, double& L, double& y, double& w) {
  const double e = ep[i];
  L = y = w = 0.0;
  if (cf_usable(e)) {
    w = 1.0 / e;
    y = yp[i];
    L = log(fp[i] / nu_ref);
  }
}

__device__ __forceinline__ void pl_term(double (&s)[6], double A, double alpha, double L, double y,
                                        double w) {
  const double p = exp(alpha * L), m = A * p;
  const double r = (y - m) * w;
  const double ja = -p * w, jb = -m * L * w;
  s[0] = fma(r, r, s[0]);
  s[1] = fma(r, ja, s[1]);
  s[2] = fma(r, jb, s[2]);
  s[3] = fma(ja, ja, s[3]);
  s[4] = fma(ja, jb, s[4]);
  s[5] = fma(jb, jb, s[5]);
}

template <int NJ>
__device__ __forceinline__ PlSums pl_eval(const PlRow<NJ>& R, int lane, double A, double alpha) {
  double s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if constexpr (NJ > 0) {
#pragma unroll
    for (int j = 0; j < NJ; ++j) pl_term(s, A, alpha, R.L[j], R.y[j], R.w[j]);
  } else {
    for (int i = lane; i < R.n; i += 64) {
      double L, y, w;
      pl_point(R.yp, R.ep, R.fp, i, R.nu_ref, L, y, w);
      pl_term(s, A, alpha, L, y, w);
    }
  }
  PlSums e;
  e.chi2 = lane0(wave_sum(s[0]));
  e.g0 = lane0(wave_sum(s[1]));
  e.g1 = lane0(wave_sum(s[2]));
  e.h00 = lane0(wave_sum(s[3]));
  e.h01 = lane0(wave_sum(s[4]));
  e.h11 = lane0(wave_sum(s[5]));
  return e;
}

// MINPACK's column norm for the scaling: 1 for a zero (or non-finite) column
__device__ __forceinline__ double pl_colnorm(double h) {
  const double c = sqrt(h);
  return (c > 0.0 && isfinite(c)) ? c : 1.0;
}

// (a b; b c) d = -(g0, g1) by its Cholesky factor; false unless positive definite
__device__ __forceinline__ bool pl_solve(double a, double b, double c, double g0, double g1,
                                         double& d0, double& d1) {
  if (!(a > 0.0)) return false;
  const double l = b / a, s = c - l * b;
  if (!(s > 0.0)) return false;
  d1 = (l * g0 - g1) / s;
  d0 = (-g0 - b * d1) / a;
  return true;
}

}  // namespace

template <int NJ>
__global__ __launch_bounds__(kBlock) void k_powlaw_fit(PowlawArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (r >= a.nrow) return;  // whole waves: nothing below synchronises the block
  const int n = a.n;
  PlRow<NJ> R;
  R.yp = a.y + (size_t)r * n;
  R.ep = a.errs + (size_t)r * n;
  R.fp = a.freqs + (size_t)r * n;
  R.nu_ref = a.nu_ref[r];
  R.n = n;

  // the one pass that counts the usable points and looks at their values
  double cnt = 0.0, bad = 0.0;
  if constexpr (NJ > 0) {
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int i = lane + 64 * j;
      R.L[j] = R.y[j] = R.w[j] = 0.0;
      if (i < n) {
        const double e = R.ep[i];
        if (cf_usable(e)) {
          const double f = R.fp[i], y = R.yp[i];
          cnt += 1.0;
          if (!isfinite(y) || !(f > 0.0) || !isfinite(f)) bad += 1.0;
          pl_point(R.yp, R.ep, R.fp, i, R.nu_ref, R.L[j], R.y[j], R.w[j]);
        }
      }
    }
  } else {
    for (int i = lane; i < n; i += 64) {
      const double e = R.ep[i];
      if (cf_usable(e)) {
        const double f = R.fp[i], y = R.yp[i];
        cnt += 1.0;
        if (!isfinite(y) || !(f > 0.0) || !isfinite(f)) bad += 1.0;
      }
    }
  }
  const int n_used = (int)lane0(wave_sum(cnt));
  bad = lane0(wave_sum(bad));
  double* o = a.out + (size_t)r * 6;
  int* info = a.info + (size_t)r * 4;
  if (n_used < 3 || bad > 0.0 || !(R.nu_ref > 0.0) || !isfinite(R.nu_ref)) {
    if (lane == 0) {
      for (int i = 0; i < 6; ++i) o[i] = NAN;
      info[0] = PPF_CHANFIT_UNUSABLE;
      info[1] = 0;
      info[2] = n_used - 2;
      info[3] = n_used;
    }
    return;
  }
  const int dof = n_used - 2;

  // Levenberg-Marquardt (k_gauss_step's rules, two free parameters)
  double x0 = a.init[2 * r], x1 = a.init[2 * r + 1];
  PlSums E = pl_eval<NJ>(R, lane, x0, x1);
  int nfev = 1, status = 0;
  if (!isfinite(E.chi2)) status = PPF_GAUSS_NONFINITE;
  double D0 = pl_colnorm(E.h00), D1 = pl_colnorm(E.h11);
  double lambda = 1e-3, nu = 2.0;
  while (!status) {
    if (E.chi2 == 0.0) {  // an exact fit: no reduction is left to test
      status = PPF_GAUSS_FTOL;
      break;
    }
    double d0 = 0.0, d1 = 0.0;
    bool ok = false;
    for (int attempt = 0; attempt < 8 && !ok; ++attempt) {
      ok = pl_solve(E.h00 + lambda * D0 * D0, E.h01, E.h11 + lambda * D1 * D1, E.g0, E.g1, d0, d1);
      if (!ok) lambda = fmax(lambda * 10.0, 1e-6);
    }
    const double t0 = D0 * d0, t1 = D1 * d1, u0 = D0 * x0, u1 = D1 * x1;
    const double pn = fma(t1, t1, t0 * t0), xn = fma(u1, u1, u0 * u0);
    if (!ok || !isfinite(pn)) {
      status = PPF_GAUSS_SINGULAR;
      break;
    }
    // predicted reduction of chi^2: -2 g.d - d.H.d = -g.d + lambda |D d|^2
    const double pred = -fma(E.g1, d1, E.g0 * d0) + lambda * pn;
    const double n0 = lane0(x0 + d0), n1 = lane0(x1 + d1);
    const PlSums T = pl_eval<NJ>(R, lane, n0, n1);
    nfev += 1;
    const double actred =
        (isfinite(T.chi2) && 0.01 * T.chi2 < E.chi2) ? 1.0 - T.chi2 / E.chi2 : -1.0;
    const double prered = pred / E.chi2;
    const double ratio = prered != 0.0 ? actred / prered : 0.0;
    if (ratio >= 1e-4) {
      x0 = n0;
      x1 = n1;
      E = T;
      D0 = fmax(D0, pl_colnorm(T.h00));
      D1 = fmax(D1, pl_colnorm(T.h11));
      const double t = 2.0 * ratio - 1.0;
      lambda *= fmax(0.1, 1.0 - t * t * t);
      nu = 2.0;
    } else {
      lambda *= nu;
      nu *= 2.0;
    }
    lambda = lane0(lambda);
    // MINPACK's tests (lmder): ftol on the reductions, xtol on the step
    const bool cf_ = fabs(actred) <= a.ftol && prered <= a.ftol && 0.5 * ratio <= 1.0;
    const bool cx_ = sqrt(pn) <= a.xtol * sqrt(xn);
    if (cf_) status = PPF_GAUSS_FTOL;
    if (cx_) status = cf_ ? PPF_GAUSS_BOTH : PPF_GAUSS_XTOL;
    if (!status && nfev >= a.cap) status = PPF_GAUSS_MAXFEV;
  }

  if (lane == 0) {
    // lmfit's covariance with scale_covar: inv(J^T J) chi2 / dof
    double vA = 0.0, vB = 0.0, cAB = 0.0;
    const double l = E.h01 / E.h00, s = E.h11 - l * E.h01;
    if (status != PPF_GAUSS_NONFINITE && E.h00 > 0.0 && s > 0.0) {
      const double red = E.chi2 / (double)dof;
      vB = red / s;
      cAB = -l * vB;
      vA = red / E.h00 - l * cAB;
    }
    o[0] = x0;
    o[1] = vA > 0.0 ? sqrt(vA) : 0.0;
    o[2] = x1;
    o[3] = vB > 0.0 ? sqrt(vB) : 0.0;
    o[4] = cAB;
    o[5] = E.chi2;
    info[0] = status;
    info[1] = nfev;
    info[2] = dof;
    info[3] = n_used;
  }
}

template __global__ void k_powlaw_fit<0>(PowlawArgs);
template __global__ void k_powlaw_fit<1>(PowlawArgs);
template __global__ void k_powlaw_fit<2>(PowlawArgs);
template __global__ void k_powlaw_fit<4>(PowlawArgs);
template __global__ void k_powlaw_fit<8>(PowlawArgs);

// np.polyfit(x, y, 1, w=w, cov=True): a, b minimise sum (w (y - a x - b))^2.
// x and y are centred on their w^2-weighted means before the slope is formed
// (x = nu^-2 is about 1e-6 and the uncentred normal equations lose digits);
// the second pass also sums the centred values, which corrects the rounding of
// the means in b = ybar - a xbar.  The covariance is that of the normal
// equations times sum (w r)^2 / (n_used - 2).
__global__ __launch_bounds__(kBlock) void k_line_fit(int nrow, int n, const double* __restrict__ x,
                                                     const double* __restrict__ y,
                                                     const double* __restrict__ w,
                                                     double* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (r >= nrow) return;  // whole waves
  const double* xr = x + (size_t)r * n;
  const double* yr = y + (size_t)r * n;
  const double* wr = w + (size_t)r * n;
  double cnt = 0.0, bad = 0.0, sw = 0.0, swx = 0.0, swy = 0.0;
  for (int i = lane; i < n; i += 64) {
    const double wi = wr[i];
    if (cf_usable(wi)) {
      const double W = wi * wi, xi = xr[i], yi = yr[i];
      cnt += 1.0;
      if (!isfinite(xi) || !isfinite(yi)) bad += 1.0;
      sw += W;
      swx = fma(W, xi, swx);
      swy = fma(W, yi, swy);
    }
  }
  const int n_used = (int)lane0(wave_sum(cnt));
  bad = lane0(wave_sum(bad));
  sw = lane0(wave_sum(sw));
  double* o = out + (size_t)r * 8;
  if (n_used < 3 || bad > 0.0 || !isfinite(sw)) {
    if (lane == 0) {
      for (int i = 0; i < 6; ++i) o[i] = NAN;
      o[6] = (double)n_used;
      o[7] = (double)PPF_CHANFIT_UNUSABLE;
    }
    return;
  }
  const double xm = lane0(wave_sum(swx)) / sw, ym = lane0(wave_sum(swy)) / sw;
  double sxx = 0.0, sxy = 0.0, sdx = 0.0, sdy = 0.0;
  for (int i = lane; i < n; i += 64) {
    const double wi = wr[i];
    if (cf_usable(wi)) {
      const double W = wi * wi, dx = xr[i] - xm, dy = yr[i] - ym;
      sxx = fma(W * dx, dx, sxx);
      sxy = fma(W * dx, dy, sxy);
      sdx = fma(W, dx, sdx);
      sdy = fma(W, dy, sdy);
    }
  }
  sxx = lane0(wave_sum(sxx));
  sxy = lane0(wave_sum(sxy));
  const double cx = lane0(wave_sum(sdx)) / sw, cy = lane0(wave_sum(sdy)) / sw;
  if (!(sxx > 0.0) || !isfinite(sxx)) {  // every usable x the same: no slope
    if (lane == 0) {
      for (int i = 0; i < 6; ++i) o[i] = NAN;
      o[6] = (double)n_used;
      o[7] = (double)PPF_GAUSS_SINGULAR;
    }
    return;
  }
  const double sa = sxy / sxx;
  double s2 = 0.0;
  for (int i = lane; i < n; i += 64) {
    const double wi = wr[i];
    if (cf_usable(wi)) {
      const double res = ((yr[i] - ym) - cy) - sa * ((xr[i] - xm) - cx);
      const double wres = wi * res;
      s2 = fma(wres, wres, s2);
    }
  }
  s2 = lane0(wave_sum(s2));
  if (lane == 0) {
    const double xbar = xm + cx;
    const double fac = s2 / (double)(n_used - 2);
    o[0] = sa;
    o[1] = fma(-sa, xm, ym) + (cy - sa * cx);
    o[2] = fac / sxx;
    o[3] = fac * (1.0 / sw + xbar * xbar / sxx);
    o[4] = -fac * xbar / sxx;
    o[5] = s2;
    o[6] = (double)n_used;
    o[7] = 0.0;
  }
}

}  // namespace ppf
