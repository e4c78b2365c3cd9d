// ppfit_nbscat.hip -- narrowband phase + scattering fits (gfx950).
//
// k_nbscat: fit_portrait_full (pptoaslib.py:928-1096) on a one-channel
// portrait with fit_flags [1, 0, 0, 1, 0] and nu_fits = nu_outs = the
// channel's own frequency, for every profile of a get_narrowband_TOAs call
// (the call the reference leaves commented out, pptoas.py:982-988).  Each
// problem has two parameters, the phase phi and t = tau or log10 tau (tau in
// rotations at the channel's frequency), and nbin / 2 harmonics.
//
// One profile per wave, from its spectrum to its result row:
//   - the wave reads D_k and M_k once (k = 1 .. nbin / 2; the DC term is
//     dropped, F0_fact = 0) and keeps X_k = D_k conj(M_k) / s^2 and
//     m_k = |M_k|^2 / s^2, s = sigma sqrt(nbin / 2), in registers: lane l owns
//     k = 1 + l + 64 j, j < NJ (48 doubles a lane at nbin 2048; under the
//     128-VGPR bound the compiler backs the larger NJ with scratch, DESIGN
//     section 14).  Above 2048 bins (NJ = 0) the rows are read again from L2
//     in every evaluation;
//   - an evaluation forms the nine sums that f, its gradient and its Hessian
//     need (pptoaslib.py:525-643 for one channel): a lane adds its harmonics
//     in j order, then one wave_sum each.  No LDS and no barrier anywhere;
//   - scipy's trust-ncg (gtol = -1, maxiter 200 * 5: the reference's x0 has
//     five entries) runs on wave-uniform scalars, every lane the same
//     control flow, as k_solve restates it (ppfit_fit.hip) for 5 parameters;
//   - the post-fit is fit_portrait_full_function_2deriv_with_scales
//     (pptoaslib.py:645-731) for one channel: the 2 x 2 covariance of
//     (phi, t), the scale and its error, snr, red_chi2 with dof = nbin - 3.
// Every sum has a fixed order inside the wave, so a profile's row is bitwise
// independent of what shares the call.
//
// Starting point.  tau0 <= 0 (or NaN) starts at 1 / nbin in both
// parameterisations (the reference does so for log10 tau only; with linear
// tau its Hessian is singular at 0).  The starting phase is the largest value
// of the cross-correlation between the profile and the template scattered at
// the starting tau, both limited to their first min(nbin / 2, 128) harmonics,
// over the phases -0.5 + g / G, g < G = min(nbin, 256) (the lowest g on a
// tie).
#include "ppfit_kernels.hpp"

namespace ppf {

namespace {

constexpr int kNbGridMax = 256;            // phases of the starting grid
constexpr int kNbGridPer = kNbGridMax / 64;  // ... a lane
constexpr int kNbGridSlots = 2;            // harmonic slots (of 64) it uses
constexpr int kNbMaxIter = 1000;           // scipy: len(x0) * 200, x0 of five

// The sums of one evaluation (all over k >= 1, already divided by s^2), with
// u = W conj(B), v = u conj(B), z = v conj(B), W = X e^{2 pi i k phi},
// B = 1 / (1 + i c tau), c = 2 pi k, q = |B|^2:
//   0 C    = sum Re u            3 C_t   = sum -c Im v        6 S    = sum m q
//   1 C_p  = sum -c Im u         4 C_pt  = sum -c^2 Re v      7 S_t  = sum m q'
//   2 C_pp = sum -c^2 Re u       5 C_tt  = sum -2 c^2 Re z    8 S_tt = sum m q''
// (derivatives with respect to phi and the linear tau; q' = -2 c^2 tau q^2,
// q'' = -2 c^2 q^2 + 8 c^4 tau^2 q^3).  tau: the linear tau they were taken at.
struct NbSums {
  double s[9];
  double tau;
};

// f, gradient and Hessian in (phi, t) from the sums (pptoaslib.py:525-643 for
// one channel); t = log10 tau brings d tau / dt = ln10 tau and its derivative
struct NbFgh {
  double f, g0, g1, h00, h01, h11;
};

struct NbChain {
  double dC0, dC1, dS1, cc00, cc01, cc11, ss11;
};

__device__ __forceinline__ NbChain nb_chain(const NbSums& e, bool log10_tau) {
  const double J = log10_tau ? kLn10 * e.tau : 1.0;
  const double J2 = log10_tau ? kLn10 * kLn10 * e.tau : 0.0;
  NbChain c;
  c.dC0 = e.s[1];
  c.dC1 = e.s[3] * J;
  c.dS1 = e.s[7] * J;
  c.cc00 = e.s[2];
  c.cc01 = e.s[4] * J;
  c.cc11 = e.s[5] * J * J + e.s[3] * J2;
  c.ss11 = e.s[8] * J * J + e.s[7] * J2;
  return c;
}

__device__ __forceinline__ NbFgh nb_fgh(const NbSums& e, bool log10_tau) {
  const NbChain c = nb_chain(e, log10_tau);
  const double C = e.s[0], S = e.s[6];
  const double A = C * C / S;
  NbFgh r;
  r.f = -A;
  r.g0 = -A * (2.0 * c.dC0 / C);
  r.g1 = -A * (2.0 * c.dC1 / C - c.dS1 / S);
  r.h00 = -2.0 * A * (c.cc00 / C + c.dC0 * c.dC0 / (C * C));
  r.h01 = -2.0 * A * (c.cc01 / C + c.dC0 * c.dC1 / (C * C) - c.dC0 * c.dS1 / (C * S));
  r.h11 = -2.0 * A * (c.cc11 / C - 0.5 * c.ss11 / S + c.dC1 * c.dC1 / (C * C) +
                      c.dS1 * c.dS1 / (S * S) - 2.0 * c.dC1 * c.dS1 / (C * S));
  return r;
}

// one harmonic's terms into a lane's partial sums
__device__ __forceinline__ void nb_term(double (&p)[9], double k, double tau, double xr, double xi,
                                        double m, double2 ph) {
  const double c = 2.0 * kPi * k, a = c * tau, c2 = c * c;
  const double q = 1.0 / fma(a, a, 1.0);
  const double2 W = cmul(cmk(xr, xi), ph);
  const double2 Bc = cmk(q, a * q);  // conj(B) = (1 + i a) q
  const double2 u = cmul(W, Bc), v = cmul(u, Bc), z = cmul(v, Bc);
  p[0] += u.x;
  p[1] -= c * u.y;
  p[2] -= c2 * u.x;
  p[3] -= c * v.y;
  p[4] -= c2 * v.x;
  p[5] -= 2.0 * c2 * z.x;
  const double q2 = q * q;
  p[6] = fma(m, q, p[6]);
  p[7] -= m * (2.0 * c2 * tau * q2);
  p[8] += m * (c2 * q2 * (8.0 * a * a * q - 2.0));
}

// The resident rows of a wave: NJ slots of 64 harmonics in registers, or
// (NJ = 0) the spectra in memory with the factor 1 / s^2
template <int NJ>
struct NbRows {
  double xr[NJ > 0 ? NJ : 1], xi[NJ > 0 ? NJ : 1], m[NJ > 0 ? NJ : 1];
  const double2* D;
  const double2* M;
  double ie2;
  int nh;  // harmonics k = 1 .. nh
};

template <int NJ>
__device__ __forceinline__ NbSums nb_eval(const NbRows<NJ>& R, int lane, double phi, double t,
                                          bool log10_tau) {
  const double tau = log10_tau ? pow(10.0, t) : t;
  double p[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  // e^{2 pi i k phi} for k = 1 + lane + 64 j by recurrence over j
  double2 ph = turn_phasor((double)(1 + lane), phi);
  const double2 step = turn_phasor(64.0, phi);
  if constexpr (NJ > 0) {
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      nb_term(p, (double)(1 + lane + 64 * j), tau, R.xr[j], R.xi[j], R.m[j], ph);
      ph = cmul(ph, step);
    }
  } else {
    for (int k = 1 + lane; k <= R.nh; k += 64) {
      const double2 d = R.D[k], mm = R.M[k];
      const double2 x = cscale(cmulc(d, mm), R.ie2);
      nb_term(p, (double)k, tau, x.x, x.y, cabs2(mm) * R.ie2, ph);
      ph = cmul(ph, step);
    }
  }
  NbSums e;
#pragma unroll
  for (int i = 0; i < 9; ++i) e.s[i] = lane0(wave_sum(p[i]));
  e.tau = lane0(tau);
  return e;
}

// phase_transform's wrap into [-0.5, 0.5) (pptoaslib.py:1040-1043)
__device__ __forceinline__ double nb_wrap_half(double p) {
  if (fabs(p) >= 0.5) {
    p = fmod(p, 1.0);
    if (p < 0.0) p += 1.0;
  }
  if (p >= 0.5) p -= 1.0;
  return p;
}

// m(p) = f + g.p + 0.5 p.(H p)
__device__ __forceinline__ double nb_model(const NbFgh& F, double p0, double p1) {
  const double b0 = F.h00 * p0 + F.h01 * p1, b1 = F.h01 * p0 + F.h11 * p1;
  return F.f + (F.g0 * p0 + F.g1 * p1) + 0.5 * (p0 * b0 + p1 * b1);
}

// ||z + t d|| = tr, the sorted roots (scipy's get_boundaries_intersections)
__device__ __forceinline__ void nb_boundary(double z0, double z1, double d0, double d1, double tr,
                                            double& ta, double& tb) {
  const double a = d0 * d0 + d1 * d1, b = 2.0 * (z0 * d0 + z1 * d1);
  const double c = z0 * z0 + z1 * z1 - tr * tr;
  const double sq = sqrt(b * b - 4.0 * a * c);
  const double aux = b + copysign(sq, b);
  double t1 = -aux / (2.0 * a), t2 = -2.0 * c / aux;
  if (t1 > t2) { const double t = t1; t1 = t2; t2 = t; }
  ta = t1;
  tb = t2;
}

// CG-Steihaug as in scipy's CGSteihaugSubproblem.solve, two parameters
__device__ __forceinline__ void nb_steihaug(const NbFgh& F, double tr, double& p0, double& p1,
                                            bool& hits) {
  const double jm = sqrt(F.g0 * F.g0 + F.g1 * F.g1);
  const double tol = fmin(0.5, sqrt(jm)) * jm;
  p0 = p1 = 0.0;
  hits = false;
  if (jm < tol) return;
  double z0 = 0.0, z1 = 0.0, r0 = F.g0, r1 = F.g1, d0 = -F.g0, d1 = -F.g1;
  for (int it = 0; it < 64; ++it) {  // a 2-D CG ends well before this
    const double B0 = F.h00 * d0 + F.h01 * d1, B1 = F.h01 * d0 + F.h11 * d1;
    const double dBd = d0 * B0 + d1 * B1;
    if (dBd <= 0.0) {
      double ta, tb;
      nb_boundary(z0, z1, d0, d1, tr, ta, tb);
      const double a0 = z0 + ta * d0, a1 = z1 + ta * d1, b0 = z0 + tb * d0, b1 = z1 + tb * d1;
      hits = true;
      const bool first = nb_model(F, a0, a1) < nb_model(F, b0, b1);
      p0 = first ? a0 : b0;
      p1 = first ? a1 : b1;
      return;
    }
    const double r2 = r0 * r0 + r1 * r1;
    const double alpha = r2 / dBd;
    const double n0 = z0 + alpha * d0, n1 = z1 + alpha * d1;
    if (sqrt(n0 * n0 + n1 * n1) >= tr) {
      double ta, tb;
      nb_boundary(z0, z1, d0, d1, tr, ta, tb);
      hits = true;
      p0 = z0 + tb * d0;
      p1 = z1 + tb * d1;
      return;
    }
    const double q0 = r0 + alpha * B0, q1 = r1 + alpha * B1;
    const double q2 = q0 * q0 + q1 * q1;
    if (sqrt(q2) < tol) {
      p0 = n0;
      p1 = n1;
      return;
    }
    const double beta = q2 / r2;
    d0 = -q0 + beta * d0;
    d1 = -q1 + beta * d1;
    z0 = n0;
    z1 = n1;
    r0 = q0;
    r1 = q1;
  }
  p0 = z0;
  p1 = z1;
}

// the starting phase (file header): every lane gets it
template <int KJ>
__device__ __forceinline__ double nb_grid_phase(const double (&yr)[KJ], const double (&yi)[KJ],
                                                int lane, int nbin) {
  const int G = nbin < kNbGridMax ? nbin : kNbGridMax;
  double2 e[kNbGridPer], ph[kNbGridPer];
  double corr[kNbGridPer];
#pragma unroll
  for (int m = 0; m < kNbGridPer; ++m) {
    const int g = lane + 64 * m;
    e[m] = turn_phasor(1.0, -0.5 + (double)g / (double)G);
    ph[m] = e[m];  // e^{2 pi i k phi_g}, k = 1
    corr[m] = 0.0;
  }
#pragma unroll
  for (int j = 0; j < KJ; ++j) {
    for (int l = 0; l < 64; ++l) {  // k = 1 + l + 64 j ascending
      const double ar = lane_of(yr[j], l), ai = lane_of(yi[j], l);
#pragma unroll
      for (int m = 0; m < kNbGridPer; ++m) {
        corr[m] += fma(ar, ph[m].x, -ai * ph[m].y);
        ph[m] = cmul(ph[m], e[m]);
      }
    }
  }
  double best = -INFINITY;
  int gbest = kNbGridMax;
#pragma unroll
  for (int m = 0; m < kNbGridPer; ++m) {
    const int g = lane + 64 * m;
    if (g < G && corr[m] > best) {
      best = corr[m];
      gbest = g;
    }
  }
  const double top = wave_max(best);
  // the lowest grid index that reaches the maximum (all of them when the
  // correlation is NaN or -inf throughout: then g = 0)
  const double cand = (best == top && gbest < G) ? (double)gbest : (double)kNbGridMax;
  double gsel = -wave_max(-cand);
  if (!(gsel < (double)G)) gsel = 0.0;
  return -0.5 + lane0(gsel) / (double)G;
}

}  // namespace

template <int NJ>
__global__ __launch_bounds__(kBlock, 4) void k_nbscat(NbScatArgs a) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (r >= a.nprof) return;  // whole waves: nothing below synchronises the block
  const int nh = a.NH - 1, nbin = a.nbin;
  const bool lg = a.log10_tau != 0;
  const double2* Dr = a.D + (size_t)r * a.NH;
  const double2* Mr = a.M + (size_t)(a.model_idx ? a.model_idx[r] : 0) * a.NH;

  // the one pass over D and M: the resident rows, Sd and the noise power
  NbRows<NJ> R;
  R.D = Dr;
  R.M = Mr;
  R.nh = nh;
  double dd = 0.0, pnoise = 0.0;
  constexpr int KJ = kNbGridSlots < (NJ > 0 ? NJ : kNbGridSlots) ? kNbGridSlots
                                                                  : (NJ > 0 ? NJ : kNbGridSlots);
  double yr[KJ], yi[KJ];  // first harmonics of X (the starting grid)
  if constexpr (NJ > 0) {
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int k = 1 + lane + 64 * j;
      double2 d = cmk(0.0, 0.0), mm = cmk(0.0, 0.0);
      if (k <= nh) {
        d = Dr[k];
        mm = Mr[k];
      }
      const double2 x = cmulc(d, mm);
      R.xr[j] = x.x;
      R.xi[j] = x.y;
      R.m[j] = cabs2(mm);
      const double d2 = cabs2(d);
      dd += d2;
      if (k >= a.kc) pnoise += d2;
    }
  } else {
    for (int k = 1 + lane; k <= nh; k += 64) {
      const double d2 = cabs2(Dr[k]);
      dd += d2;
      if (k >= a.kc) pnoise += d2;
    }
#pragma unroll
    for (int j = 0; j < KJ; ++j) {
      const int k = 1 + lane + 64 * j;  // k <= 128 < nh here
      const double2 x = cmulc(Dr[k], Mr[k]);
      yr[j] = x.x;
      yi[j] = x.y;
    }
  }
  dd = lane0(wave_sum(dd));
  pnoise = lane0(wave_sum(pnoise));
  double noise = a.noise ? a.noise[r] : NAN;
  // get_noise_PS (pplib.py:2227-2253), as k_phase_shift
  if (isnan(noise)) noise = sqrt(pnoise / (double)nbin / (double)(a.NH - a.kc));
  const double ie2 = 1.0 / (noise * noise * (0.5 * (double)nbin));  // 1 / errs_FT^2
  R.ie2 = ie2;
  const double Sd = dd * ie2;
  if constexpr (NJ > 0) {
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      R.xr[j] *= ie2;
      R.xi[j] *= ie2;
      R.m[j] *= ie2;
    }
#pragma unroll
    for (int j = 0; j < KJ; ++j) {
      yr[j] = R.xr[j];
      yi[j] = R.xi[j];
    }
  }

  // starting point
  double tau_s = a.tau0 ? a.tau0[r] : 0.0;
  if (!(tau_s > 0.0)) tau_s = 1.0 / (double)nbin;
#pragma unroll
  for (int j = 0; j < KJ; ++j) {  // Y_k = X_k conj(B_k(tau_s)), k <= 64 KJ
    const int k = 1 + lane + 64 * j;
    const double aa = 2.0 * kPi * (double)k * tau_s, q = 1.0 / fma(aa, aa, 1.0);
    const double2 y = k <= nh ? cmul(cmk(yr[j], yi[j]), cmk(q, aa * q)) : cmk(0.0, 0.0);
    yr[j] = y.x;
    yi[j] = y.y;
  }
  double x0 = nb_grid_phase<KJ>(yr, yi, lane, nbin);
  double x1 = lane0(lg ? log10(tau_s) : tau_s);

  // scipy's _minimize_trust_region with the CG-Steihaug subproblem: E the
  // accepted point's sums, Ee those of the last evaluated point (scipy's
  // ScalarFunction memoises it: a proposal bitwise equal to it is not
  // evaluated again and does not count in nfev)
  NbSums E, Ee;
  double n0 = x0, n1 = x1, e0 = 0.0, e1 = 0.0, tr = 1.0, predv = 0.0;
  bool hits = false, started = false;
  int nfev = 0, status = 0, kit = 0;
  for (;;) {
    // the objective at the proposal n (at the start: at x itself)
    if (!(started && n0 == e0 && n1 == e1)) {
      Ee = nb_eval<NJ>(R, lane, n0, n1, lg);
      e0 = n0;
      e1 = n1;
      nfev += 1;
    }
    if (!started) {
      E = Ee;
      started = true;
    } else {
      const double f = -(E.s[0] * E.s[0] / E.s[6]), fp = -(Ee.s[0] * Ee.s[0] / Ee.s[6]);
      const double actual = f - fp, pred = f - predv;
      if (pred <= 0.0) {
        status = 2;
        break;
      }
      const double rho = actual / pred;
      if (rho < 0.25) tr *= 0.25;
      else if (rho > 0.75 && hits) tr = fmin(2.0 * tr, 1000.0);
      tr = lane0(tr);
      if (rho > 0.15) {
        x0 = n0;
        x1 = n1;
        E = Ee;
      }
      kit += 1;
      if (kit >= kNbMaxIter) {
        status = 1;
        break;
      }
    }
    const NbFgh F = nb_fgh(E, lg);
    const double jm = sqrt(F.g0 * F.g0 + F.g1 * F.g1);
    if (!(jm >= -1.0)) {  // NaN: scipy's loop condition fails
      status = 0;
      break;
    }
    double p0, p1;
    nb_steihaug(F, tr, p0, p1, hits);
    predv = lane0(nb_model(F, p0, p1));
    n0 = lane0(x0 + p0);
    n1 = lane0(x1 + p1);
  }

  // post-fit (pptoaslib.py:645-731 and 1045-1096 for one channel)
  if (lane == 0) {
    const NbChain c = nb_chain(E, lg);
    const double C = E.s[0], S = E.s[6];
    const double A = C * C / S, scale = C / S, f = -A;
    const double H00 = -2.0 * A * (c.cc00 / C);
    const double H01 = -2.0 * A * (c.cc01 / C);
    const double H11 = -2.0 * A * (c.cc11 / C - 0.5 * c.ss11 / S);
    const double U0 = -2.0 * c.dC0, U1 = -2.0 * (c.dC1 - scale * c.dS1);
    const double Ci = 1.0 / (2.0 * S);
    const double X00 = H00 - U0 * U0 * Ci, X01 = H01 - U0 * U1 * Ci, X11 = H11 - U1 * U1 * Ci;
    const double det = X00 * X11 - X01 * X01;
    const double I00 = X11 / det, I01 = -X01 / det, I11 = X00 / det;
    const double uxu = U0 * (I00 * U0 + I01 * U1) + U1 * (I01 * U0 + I11 * U1);
    const double LR = Ci * Ci * uxu + Ci;
    const double chi2 = Sd + f;
    double* o = a.out + (size_t)r * 9;
    o[0] = nb_wrap_half(x0);
    o[1] = sqrt(2.0 * I00);
    o[2] = x1;
    o[3] = sqrt(2.0 * I11);
    o[4] = scale;
    o[5] = sqrt(2.0 * LR);
    o[6] = scale * sqrt(S);
    o[7] = chi2 / (double)(nbin - 3);
    o[8] = 2.0 * I01;
    a.status[r] = status;
    a.nfev[r] = nfev;
  }
}

template __global__ void k_nbscat<0>(NbScatArgs);
template __global__ void k_nbscat<1>(NbScatArgs);
template __global__ void k_nbscat<2>(NbScatArgs);
template __global__ void k_nbscat<4>(NbScatArgs);
template __global__ void k_nbscat<8>(NbScatArgs);
template __global__ void k_nbscat<16>(NbScatArgs);

}  // namespace ppf
