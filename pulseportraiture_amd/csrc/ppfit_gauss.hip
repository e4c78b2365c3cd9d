// ppfit_gauss.hip -- batched Levenberg-Marquardt fits of Gaussian-component
// portraits (ppgauss model building; fit_gaussian_portrait, pplib.py:1924-2052,
// and fit_gaussian_profile, pplib.py:1842-1922).
//
// The residual is the reference's (pplib.py:1230-1242): (data -
// gen_gaussian_portrait(...)) / errs, the portrait exactly as k_gauss_port
// builds it (bin-centre wrap, |z| < 20 support, rescale factor, evolve codes 0
// and 1), scattered per channel by 1 / (1 + 2 pi i k tau_n), tau_n = tau / nbin
// (f_n / nu_ref)^alpha.  The Jacobian is analytic: amp_n fact exp(-z^2 / 2) is
// differentiated on its support with fact, the wrap and the support held fixed
// (they are piecewise constant).
//
// Joint fits of several receivers (JOIN instantiations; fit_gaussian_portrait
// with join_params, pplib.py:923-929, 1992-2001): row n of join group g is the
// model row rotated as rotate_data does it, every model-side spectrum times
// R_k = exp(2 pi i k theta_n), theta_n = phase_g + DM_g dm_coef[n].  Its
// derivative to theta_n is one more Gram row, 2 pi i k R_k S_k X_k; phase_g
// and DM_g reach it through the chain-rule scalars [join_of[n] == g] and
// [join_of[n] == g] dm_coef[n].  The no-join instantiations do the arithmetic
// they did before there was a JOIN flag.
//
//   k_gauss_basis  per (portrait, channel) row: the unscattered model row and
//                  three derivative profiles per component (d/dloc_n,
//                  d/dwid_n, d/damp_n) in the time domain, the chain-rule
//                  scalars from the evolved to the external parameters, tau_n
//                  (JOIN: and the join parameters' scalars);
//   (k_rfft_rows   the existing row transform, forward only)
//   k_gauss_gram   per row, on the spectra (Parseval, DC and Nyquist weights
//                  folded in): the Gram matrix of K = 3 ngauss + 3 rows --
//                  the residual, the constant, the tau_n derivative and the
//                  scattered derivative profiles (JOIN: all rotated, and the
//                  theta_n derivative as row K) -- so chi^2, J^T r and
//                  J^T J of the row come from one product;
//   k_gauss_init   external -> internal parameters (lmfit's MINUIT bound
//                  transforms), free-parameter count, evaluation cap;
//   k_gauss_step   one workgroup per portrait: the chain rule and the sum
//                  over channels in channel order, then (fits) the gain
//                  ratio test of the trial point, the stopping rules and the
//                  next Levenberg-Marquardt step from a Cholesky in LDS; on
//                  termination the covariance.
//
// Every sum runs in a fixed order inside one thread and a portrait's
// launches read nothing of another portrait: results are bitwise
// reproducible and independent of what else shares the call.  No atomics.
#include "ppfit_kernels.hpp"

namespace ppf {

__device__ __forceinline__ double gf_py_mod1(double x) {
  double m = fmod(x, 1.0);
  if (m != 0.0) {
    if (m < 0.0) m += 1.0;
  } else {
    m = 0.0;
  }
  return m;
}

// bin centre j wrapped to within half a turn of mean (pplib.py:801-805), as
// k_gauss_port's locval
__device__ __forceinline__ double gf_locval(int j, int nbin, double start, double stop, double step,
                                            double mean) {
  double x = (j == nbin - 1) ? stop : __dadd_rn(__dmul_rn((double)j, step), start);
  if (mean < 0.5) {
    if (x > mean + 0.5) x -= 1.0;
  } else if (x < mean - 0.5) {
    x += 1.0;
  }
  return x;
}

// evolve_parameter (pplib.py:1030-1046) with its derivatives to the value
// (dp) and to the evolution parameter (de)
__device__ __forceinline__ double gf_evolve(int code, double lr, double df, double par, double evo,
                                            double& dp, double& de) {
  if (code == 0) {  // power law: exp(ln(f / nu_ref) idx + ln par)
    const double v = exp(__dadd_rn(__dmul_rn(lr, evo), log(par)));
    dp = exp(__dmul_rn(lr, evo));
    de = v * lr;
    return v;
  }
  dp = 1.0;
  de = df;
  return __dadd_rn(__dmul_rn(df, evo), par);  // linear
}

// lmfit's bounds (pplib.py:1964-2001): 1 lower only (tau, amp >= 0), 2
// two-sided (0 <= wid <= wid_max), 0 none (JOIN: the join parameters,
// 2 + 6 ngauss <= q < npar - 1, among them)
template <bool JOIN>
__device__ __forceinline__ int gf_kind(int q, int npar, int ngauss) {
  if (q == 1) return 1;
  if (q < 2 || q == npar - 1) return 0;
  if constexpr (JOIN)
    if (q >= 2 + 6 * ngauss) return 0;
  const int m = (q - 2) % 6;
  return m == 2 ? 2 : (m == 4 ? 1 : 0);
}
// MINUIT transforms as lmfit applies them (lower bound 0 throughout)
__device__ __forceinline__ double gf_to_ext(int kind, double x, double hi) {
  if (kind == 1) return -1.0 + sqrt(x * x + 1.0);
  if (kind == 2) return (sin(x) + 1.0) * hi / 2.0;
  return x;
}
__device__ __forceinline__ double gf_dext(int kind, double x, double hi) {
  if (kind == 1) return x / sqrt(x * x + 1.0);
  if (kind == 2) return cos(x) * hi / 2.0;
  return 1.0;
}
__device__ __forceinline__ double gf_to_int(int kind, double v, double hi) {
  if (kind == 1) {
    v = fmax(v, 0.0);
    return sqrt((v + 1.0) * (v + 1.0) - 1.0);
  }
  if (kind == 2) {
    v = fmin(fmax(v, 0.0), hi);
    return asin(2.0 * v / hi - 1.0);
  }
  return v;
}

// the Gram row of external parameter q: 1 the constant, 2 the tau_n
// derivative, 3 + 3 c + {0 loc, 1 wid, 2 amp}, 3 + 3 ngauss the theta_n
// derivative (JOIN: phase_g and DM_g of every join group)
template <bool JOIN>
__device__ __forceinline__ int gf_basis(int q, int npar, int ngauss) {
  if (q == 0) return 1;
  if (q == 1 || q == npar - 1) return 2;
  if constexpr (JOIN)
    if (q >= 2 + 6 * ngauss) return 3 + 3 * ngauss;
  return 3 + 3 * ((q - 2) / 6) + ((q - 2) % 6) / 2;
}
__device__ __forceinline__ int gf_tri(int i, int j) {  // packed lower triangle, i >= j
  return i * (i + 1) / 2 + j;
}

// grid (nchan, nport)
template <bool JOIN>
__global__ __launch_bounds__(256) void k_gauss_basis(GaussFitArgs a) {
  constexpr int NT = 256;
  const int n = blockIdx.x, p = blockIdx.y;
  if (a.state && a.state[p].done) return;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int nbin = a.nbin, npar = a.npar, KT = 1 + 3 * a.ngauss;
  const size_t row = (size_t)p * a.nchan + n;
  const double* par = a.pext + (size_t)p * npar;
  const int* code = a.code + 3 * p;
  const double f = a.freqs[row], nu_ref = a.nu_ref[p];
  const double lr = log(f) - log(nu_ref), df = f - nu_ref;
  double* T = a.rows + row * KT * nbin;
  double* cf = a.coef + row * npar;
  __shared__ double s_max[NT / 64];
  __shared__ int s_arg[NT / 64];
  const double start = 0.5 / (double)nbin, stop = 1.0 - 0.5 / (double)nbin;
  const double step = (stop - start) / (double)(nbin - 1);
  constexpr int QMAX = 32;  // nbin <= 8192 = 32 x 256
  double model[QMAX];
  const int nq = (nbin + NT - 1) / NT;
  const double dc = par[0];
#pragma unroll
  for (int q = 0; q < QMAX; ++q) model[q] = dc;
  if (tid == 0) {
    // tau_n = tau / nbin (f / nu_ref)^alpha and its derivatives to tau, alpha
    const double pw = pow(f / nu_ref, par[npar - 1]);
    const double tn = par[1] / (double)nbin * pw;
    a.taun[row] = tn;
    cf[0] = 1.0;
    cf[1] = pw / (double)nbin;
    cf[npar - 1] = tn * log(f / nu_ref);
  }
  if constexpr (JOIN) {
    // d theta_n / d phase_g, d theta_n / d DM_g
    if (tid < 2 * a.njoin) {
      const bool mine = a.join_of[row] == (tid >> 1);
      cf[2 + 6 * a.ngauss + tid] = mine ? ((tid & 1) ? a.dm_coef[row] : 1.0) : 0.0;
    }
  }
  for (int c = 0; c < a.ngauss; ++c) {
    const double* q6 = par + 2 + 6 * c;
    double dp[3], de[3];
    const double loc = gf_evolve(code[0], lr, df, q6[0], q6[1], dp[0], de[0]);
    const double wid = gf_evolve(code[1], lr, df, q6[2], q6[3], dp[1], de[1]);
    const double amp = gf_evolve(code[2], lr, df, q6[4], q6[5], dp[2], de[2]);
    if (tid < 6) cf[2 + 6 * c + tid] = (tid & 1) ? de[tid >> 1] : dp[tid >> 1];
    double* Tl = T + (size_t)(1 + 3 * c) * nbin;
    double* Tw = Tl + nbin;
    double* Ta = Tw + nbin;
    if (!(wid > 0.0)) {  // adds zeros (k_gauss_port): no derivative either
      for (int j = tid; j < nbin; j += NT) Tl[j] = Tw[j] = Ta[j] = 0.0;
      continue;
    }
    const double sigma = wid / a.fwhm;
    const double mean = gf_py_mod1(loc);
    const double norm = __dmul_rn(sigma, a.sqrt2pi);
    double best = -1.0;
    int bi = nbin;
    double rv[QMAX];
#pragma unroll
    for (int q = 0; q < QMAX; ++q) {
      rv[q] = 0.0;
      const int j = tid + NT * q;
      if (q < nq && j < nbin) {
        const double z = (gf_locval(j, nbin, start, stop, step, mean) - mean) / sigma;
        const double v = (fabs(z) < 20.0) ? exp(__dmul_rn(-0.5, __dmul_rn(z, z))) / norm : 0.0;
        rv[q] = v;
        if (v > best) { best = v; bi = j; }
      }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      const double ob = __shfl_xor(best, o);
      const int oi = __shfl_xor(bi, o);
      if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
    }
    if (lane == 0) { s_max[w] = best; s_arg[w] = bi; }
    __syncthreads();
    double gb = s_max[0];
    int gi = s_arg[0];
    for (int v = 1; v < NT / 64; ++v)
      if (s_max[v] > gb || (s_max[v] == gb && s_arg[v] < gi)) { gb = s_max[v]; gi = s_arg[v]; }
    __syncthreads();
    double fact = 1.0;
    const bool scale = gb != 0.0 && gi < nbin;
    if (scale) {
      const double z = (gf_locval(gi, nbin, start, stop, step, mean) - loc) / sigma;
      fact = exp(__dmul_rn(-0.5, __dmul_rn(z, z))) / gb;
    }
#pragma unroll
    for (int q = 0; q < QMAX; ++q) {
      const int j = tid + NT * q;
      if (q < nq && j < nbin) {
        const double prof = scale ? __dmul_rn(fact, rv[q]) : rv[q];
        model[q] = __dadd_rn(model[q], __dmul_rn(amp, prof));
        const double z = (gf_locval(j, nbin, start, stop, step, mean) - mean) / sigma;
        const double ap = amp * prof;
        Tl[j] = ap * z / sigma;
        Tw[j] = ap * z * z / wid;
        Ta[j] = prof;
      }
    }
  }
#pragma unroll
  for (int q = 0; q < QMAX; ++q) {
    const int j = tid + NT * q;
    if (q < nq && j < nbin) T[j] = model[q];
  }
}

// grid (nchan, nport): G[row][tri(i, j)] = <B_i, B_j> / err^2 over the bins,
// formed on the spectra.  B_0 the residual, B_1 the constant, B_2 the tau_n
// derivative, B_3.. the scattered derivative profiles.
constexpr int kGfTile = 32;                        // harmonics per LDS tile
constexpr int kGfStride = 2 * kGfTile + 1;         // odd row stride: no bank conflicts
constexpr int kGfMaxBasis = 3 * kFitMaxGauss + 3;  // 51
// pairs of one thread: 6 without and with the join row (1326 and 1378 pairs)
constexpr int kGfPairsPerThread = (kGfMaxBasis * (kGfMaxBasis + 1) / 2 + 255) / 256;
static_assert(((kGfMaxBasis + 1) * (kGfMaxBasis + 2) / 2 + 255) / 256 == kGfPairsPerThread,
              "the join row needs no further pair per thread");

template <bool JOIN>
__global__ __launch_bounds__(256) void k_gauss_gram(GaussFitArgs a) {
  const int n = blockIdx.x, p = blockIdx.y;
  if (a.state && a.state[p].done) return;
  __shared__ double tile[(kGfMaxBasis + (JOIN ? 1 : 0)) * kGfStride];
  const int tid = threadIdx.x;
  const int nbin = a.nbin, NH = nbin / 2 + 1, KT = 1 + 3 * a.ngauss;
  const int KB = KT + 2 + (JOIN ? 1 : 0);
  const size_t row = (size_t)p * a.nchan + n;
  const double2* X = a.spec + row * KT * NH;
  const double2* D = a.dspec + row * NH;
  const double tn = a.taun[row];
  const double ierr = 1.0 / a.errs[row];
  const int npairs = KB * (KB + 1) / 2;
  double theta = 0.0;  // the row's rotation, reduced to (-1/2, 1/2]: k is an integer
  if constexpr (JOIN) {
    const double* jp = a.pext + (size_t)p * a.npar + 2 + 6 * a.ngauss + 2 * a.join_of[row];
    theta = fma(jp[1], a.dm_coef[row], jp[0]);
    theta -= rint(theta);
  }
  int pi[kGfPairsPerThread], pj[kGfPairsPerThread];
  double acc[kGfPairsPerThread];
#pragma unroll
  for (int s = 0; s < kGfPairsPerThread; ++s) {
    const int e = tid + 256 * s;
    int i = 0;
    while ((i + 1) * (i + 2) / 2 <= e) ++i;
    pi[s] = i;
    pj[s] = e - i * (i + 1) / 2;
    acc[s] = 0.0;
    if (e >= npairs) pi[s] = -1;
  }
  for (int k0 = 0; k0 < NH; k0 += kGfTile) {
    __syncthreads();
    for (int e = tid; e < KB * kGfTile; e += 256) {
      const int b = e / kGfTile, kk = e % kGfTile, k = k0 + kk;
      double2 v = cmk(0.0, 0.0);
      if (k < NH) {
        // S = 1 / (1 + 2 pi i k tau_n), dS / dtau_n = -2 pi i k S^2
        const double ak = 2.0 * M_PI * (double)k * tn;
        const double den = 1.0 / (1.0 + ak * ak);
        const double2 S = cmk(den, -ak * den);
        if (b == 0) {
          v = csub(D[k], cmul(S, X[k]));
        } else if (b == 1) {
          v = cmk(k == 0 ? (double)nbin : 0.0, 0.0);
        } else if (b == 2) {
          const double2 S2 = cmul(S, S);
          const double c2 = 2.0 * M_PI * (double)k;
          v = cmul(cmk(c2 * S2.y, -c2 * S2.x), X[k]);
        } else if (!JOIN || b < KT + 2) {
          v = cmul(S, X[(size_t)(b - 2) * NH + k]);
        }
        if constexpr (JOIN) {
          // R = exp(2 pi i k theta_n) on the model side; the theta_n
          // derivative of R S X_0 is 2 pi i k R S X_0.  The rows are rotated
          // as time series (gen_gaussian_portrait scatters, transforms back
          // and hands the rows to rotate_data): at Nyquist the scattered
          // spectrum has lost its imaginary part before R multiplies it.
          const bool nyq = 2 * k == nbin;
          double rs, rc;
          sincospi(2.0 * (double)k * theta, &rs, &rc);
          const double2 R = cmk(rc, rs);
          if (b == 0 || b == KT + 2) {
            double2 m = cmul(S, X[k]);
            if (nyq) m.y = 0.0;
            m = cmul(R, m);
            const double c2 = 2.0 * M_PI * (double)k;
            v = b == 0 ? csub(D[k], m) : cmk(-c2 * m.y, c2 * m.x);
          } else if (b >= 2) {
            if (nyq) v.y = 0.0;
            v = cmul(R, v);
          }
        }
        // Parseval: sum_j x_j y_j = (1 / nbin) sum_k w_k Re(X_k conj(Y_k)),
        // w = 1 at DC and Nyquist, 2 between
        const double sc = sqrt(((k == 0 || 2 * k == nbin) ? 1.0 : 2.0) / (double)nbin) * ierr;
        v = cscale(v, sc);
        if (2 * k == nbin || k == 0) v.y = 0.0;
      }
      tile[b * kGfStride + 2 * kk] = v.x;
      tile[b * kGfStride + 2 * kk + 1] = v.y;
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < kGfPairsPerThread; ++s) {
      if (pi[s] < 0) continue;
      const double* ti = tile + pi[s] * kGfStride;
      const double* tj = tile + pj[s] * kGfStride;
      double t = acc[s];
#pragma unroll 8
      for (int kk = 0; kk < 2 * kGfTile; ++kk) t = fma(ti[kk], tj[kk], t);
      acc[s] = t;
    }
  }
  double* G = a.gram + row * npairs;
#pragma unroll
  for (int s = 0; s < kGfPairsPerThread; ++s)
    if (pi[s] >= 0) G[tid + 256 * s] = acc[s];
}

// grid (nport), npar threads used
template <bool JOIN>
__global__ __launch_bounds__(256) void k_gauss_init(GaussFitArgs a, const double* __restrict__ init,
                                                    const int* __restrict__ flags) {
  const int p = blockIdx.x, tid = threadIdx.x, npar = a.npar;
  double* st = a.lm + (size_t)p * kGfLmDoubles;
  const double* v0 = init + (size_t)p * npar;
  const int* fl = flags + (size_t)p * npar;
  if (tid < npar) {
    const int kind = gf_kind<JOIN>(tid, npar, a.ngauss);
    const double x = gf_to_int(kind, v0[tid], a.wid_max);
    st[kGfXt + tid] = x;
    st[kGfXi + tid] = x;
    // a free parameter is evaluated at the image of its internal value
    a.pext[(size_t)p * npar + tid] = fl[tid] ? gf_to_ext(kind, x, a.wid_max) : v0[tid];
  }
  if (tid == 0) {
    int nfree = 0;
    for (int q = 0; q < npar; ++q) nfree += fl[q] != 0;
    GaussFitState s;
    s.done = 0;
    s.status = 0;
    s.nfev = 1;
    s.nfree = nfree;
    s.first = 1;
    s.cap = a.max_nfev > 0 ? a.max_nfev : 2000 * (nfree + 1);
    s.dof = a.nchan * a.nbin - nfree;
    s.pad = 0;
    a.state[p] = s;
  }
}

// Cholesky of the packed lower triangle L (LDS), all threads; false when a
// pivot is not positive
__device__ bool gf_cholesky(double* L, int nf) {
  const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
  bool ok = true;
  for (int j = 0; j < nf; ++j) {
    const double d = L[gf_tri(j, j)];
    if (!(d > 0.0) || !isfinite(d)) ok = false;
    const double sd = ok ? sqrt(d) : 1.0;
    __syncthreads();
    for (int i = j + tid; i < nf; i += 256) L[gf_tri(i, j)] = i == j ? sd : L[gf_tri(i, j)] / sd;
    __syncthreads();
    for (int i = j + 1 + ty; i < nf; i += 16) {
      const double lij = L[gf_tri(i, j)];
      for (int k = j + 1 + tx; k <= i; k += 16) L[gf_tri(i, k)] -= lij * L[gf_tri(k, j)];
    }
    __syncthreads();
  }
  return ok;
}

// v <- (L L^T)^-1 v, v in LDS, all threads
__device__ void gf_solve(const double* L, double* v, int nf) {
  const int tid = threadIdx.x;
  for (int j = 0; j < nf; ++j) {
    __syncthreads();
    const double vj = v[j] / L[gf_tri(j, j)];
    __syncthreads();
    if (tid == 0) v[j] = vj;
    for (int i = j + 1 + tid; i < nf; i += 256) v[i] -= L[gf_tri(i, j)] * vj;
  }
  for (int j = nf - 1; j >= 0; --j) {
    __syncthreads();
    const double vj = v[j] / L[gf_tri(j, j)];
    __syncthreads();
    if (tid == 0) v[j] = vj;
    for (int i = tid; i < j; i += 256) v[i] -= L[gf_tri(j, i)] * vj;
  }
  __syncthreads();
}

constexpr int kGfInFlight = 16;  // channels whose loads one thread of the channel sum overlaps

// grid (nport).  fit == 0: chi^2, J^T r, J^T J over the external parameters
// at a.pext into the outputs.  fit == 1: one Levenberg-Marquardt iteration.
template <bool JOIN>
__global__ __launch_bounds__(256) void k_gauss_step(GaussFitArgs a, int fit) {
  const int p = blockIdx.x, tid = threadIdx.x;
  if (fit && a.state[p].done) return;
  __shared__ double L[kGfMaxPar * (kGfMaxPar + 1) / 2];
  __shared__ double s_fac[kGfMaxPar], s_v[kGfMaxPar], s_x[kGfMaxPar], s_d[kGfMaxPar];
  __shared__ int s_fi[kGfMaxPar], s_free[kGfMaxPar];
  __shared__ double s_red[8];
  const int npar = a.npar, nchan = a.nchan, KB = 3 * a.ngauss + 3 + (JOIN ? 1 : 0);
  const int npairs = KB * (KB + 1) / 2;
  const double* G = a.gram + (size_t)p * nchan * npairs;
  const double* cf = a.coef + (size_t)p * nchan * npar;
  double* st = a.lm + (size_t)p * kGfLmDoubles;
  const int* fl = fit ? a.flags + (size_t)p * npar : nullptr;
  int nf = npar;
  if (fit) {
    if (tid == 0) {
      int c = 0;
      for (int q = 0; q < npar; ++q) {
        s_fi[q] = fl[q] ? c : -1;
        if (fl[q]) s_free[c++] = q;
      }
    }
    if (tid < npar)
      s_fac[tid] = gf_dext(gf_kind<JOIN>(tid, npar, a.ngauss), st[kGfXt + tid], a.wid_max);
    __syncthreads();
    nf = a.state[p].nfree;
  }
  // --- the chain rule and the sum over channels, in channel order
  double* Hout = fit ? st + kGfHt : a.jtj + (size_t)p * npar * npar;
  double* gout = fit ? st + kGfGt : a.jtr + (size_t)p * npar;
  const int ld = fit ? nf : npar;
  const int ntri = npar * (npar + 1) / 2;
  for (int e = tid; e < ntri + npar + 1; e += 256) {
    if (e < ntri) {
      int q = (int)((sqrt(8.0 * (double)e + 1.0) - 1.0) * 0.5);
      while (gf_tri(q + 1, 0) <= e) ++q;
      while (gf_tri(q, 0) > e) --q;
      const int r = e - gf_tri(q, 0);
      int iq = q, ir = r;
      if (fit) {
        iq = s_fi[q];
        ir = s_fi[r];
        if (iq < 0 || ir < 0) continue;
      }
      const int bq = gf_basis<JOIN>(q, npar, a.ngauss), br = gf_basis<JOIN>(r, npar, a.ngauss);
      const int gi = gf_tri(max(bq, br), min(bq, br));
      // kGfInFlight channels' loads in flight, added in channel order
      double s = 0.0;
      int n = 0;
      for (; n + kGfInFlight <= nchan; n += kGfInFlight) {
        double c[kGfInFlight], g[kGfInFlight];
#pragma unroll
        for (int u = 0; u < kGfInFlight; ++u) {
          c[u] = cf[(size_t)(n + u) * npar + q] * cf[(size_t)(n + u) * npar + r];
          g[u] = G[(size_t)(n + u) * npairs + gi];
        }
#pragma unroll
        for (int u = 0; u < kGfInFlight; ++u) s = fma(c[u], g[u], s);
      }
      for (; n < nchan; ++n)
        s = fma(cf[(size_t)n * npar + q] * cf[(size_t)n * npar + r], G[(size_t)n * npairs + gi], s);
      if (fit) s *= s_fac[q] * s_fac[r];
      Hout[(size_t)iq * ld + ir] = s;
      Hout[(size_t)ir * ld + iq] = s;
    } else if (e < ntri + npar) {
      const int q = e - ntri;
      if (fit && s_fi[q] < 0) continue;
      const int gi = gf_tri(gf_basis<JOIN>(q, npar, a.ngauss), 0);
      double s = 0.0;
      for (int n = 0; n < nchan; ++n) s = fma(cf[(size_t)n * npar + q], G[(size_t)n * npairs + gi], s);
      s = -s;  // r = (data - model) / err: J = -dmodel / err
      if (fit) gout[s_fi[q]] = s * s_fac[q];
      else gout[q] = s;
    } else {
      double s = 0.0;
      for (int n = 0; n < nchan; ++n) s += G[(size_t)n * npairs];
      if (fit) st[kGfSc + kGfChi2t] = s;
      else a.chi2[p] = s;
    }
  }
  if (!fit) return;
  __syncthreads();

  // --- Levenberg-Marquardt on the internal variables
  GaussFitState S = a.state[p];
  double* sc = st + kGfSc;
  const double chi2t = sc[kGfChi2t];
  double lambda = sc[kGfLambda], nu = sc[kGfNu];
  bool accept = false;
  int status = 0;
  if (S.first) {
    if (!isfinite(chi2t)) status = PPF_GAUSS_NONFINITE;
    accept = true;
    lambda = 1e-3;
    nu = 2.0;
  } else {
    const double chi2 = sc[kGfChi2];
    const double actred = (isfinite(chi2t) && 0.01 * chi2t < chi2) ? 1.0 - chi2t / chi2 : -1.0;
    const double prered = sc[kGfPred] / chi2;
    const double ratio = prered != 0.0 ? actred / prered : 0.0;
    if (ratio >= 1e-4) {
      accept = true;
      const double t = 2.0 * ratio - 1.0;
      lambda *= fmax(0.1, 1.0 - t * t * t);
      nu = 2.0;
    } else {
      lambda *= nu;
      nu *= 2.0;
    }
    // MINPACK's tests (lmder): ftol on the reductions, xtol on the step
    const bool cf_ = fabs(actred) <= a.ftol && prered <= a.ftol && 0.5 * ratio <= 1.0;
    const bool cx_ = sc[kGfPnorm] <= a.xtol * sc[kGfXnorm];
    if (cf_) status = PPF_GAUSS_FTOL;
    if (cx_) status = cf_ ? PPF_GAUSS_BOTH : PPF_GAUSS_XTOL;
    if (!status && S.nfev >= S.cap) status = PPF_GAUSS_MAXFEV;
  }
  if (accept) {  // the trial point becomes the current one
    for (int e = tid; e < nf * nf; e += 256) st[kGfHc + e] = st[kGfHt + e];
    if (tid < nf) st[kGfGc + tid] = st[kGfGt + tid];
    if (tid < npar) st[kGfXi + tid] = st[kGfXt + tid];
    if (tid < nf) {
      // MINPACK's column scaling: the running maximum of the column norms,
      // 1 for a zero column
      const double cn = sqrt(st[kGfHt + (size_t)tid * nf + tid]);
      double dg = S.first ? (cn > 0.0 ? cn : 1.0) : fmax(st[kGfDg + tid], cn);
      if (!isfinite(dg)) dg = 1.0;
      st[kGfDg + tid] = dg;
    }
  }
  __syncthreads();
  if (tid < nf) {
    s_d[tid] = st[kGfDg + tid];
    s_x[tid] = st[kGfXi + s_free[tid]];
  }
  __syncthreads();
  const double chi2 = accept ? chi2t : sc[kGfChi2];
  if (nf == 0 && !status) status = PPF_GAUSS_FTOL;

  if (!status) {
    // (H + lambda D^2) delta = -g
    bool ok = false;
    for (int attempt = 0; attempt < 8 && !ok; ++attempt) {
      for (int i = tid >> 4; i < nf; i += 16)
        for (int k = tid & 15; k <= i; k += 16)
          L[gf_tri(i, k)] = st[kGfHc + (size_t)i * nf + k] + (i == k ? lambda * s_d[i] * s_d[i] : 0.0);
      __syncthreads();
      ok = gf_cholesky(L, nf);
      if (!ok) lambda = fmax(lambda * 10.0, 1e-6);
      __syncthreads();
    }
    if (!ok) {
      status = PPF_GAUSS_SINGULAR;
    } else {
      if (tid < nf) s_v[tid] = -st[kGfGc + tid];
      __syncthreads();
      gf_solve(L, s_v, nf);
      if (tid == 0) {
        double gd = 0.0, pn = 0.0, xn = 0.0;
        for (int i = 0; i < nf; ++i) {
          gd = fma(st[kGfGc + i], s_v[i], gd);
          const double t = s_d[i] * s_v[i], u = s_d[i] * s_x[i];
          pn = fma(t, t, pn);
          xn = fma(u, u, xn);
        }
        // predicted reduction of chi^2: -2 g.d - d.H.d = -g.d + lambda |D d|^2
        sc[kGfPred] = -gd + lambda * pn;
        sc[kGfPnorm] = sqrt(pn);
        sc[kGfXnorm] = sqrt(xn);
        s_red[0] = isfinite(pn) ? 1.0 : 0.0;
      }
      __syncthreads();
      if (s_red[0] == 0.0) {
        status = PPF_GAUSS_SINGULAR;
      } else if (tid < nf) {
        const int q = s_free[tid];
        const double x = s_x[tid] + s_v[tid];
        st[kGfXt + q] = x;
        a.pext[(size_t)p * npar + q] = gf_to_ext(gf_kind<JOIN>(q, npar, a.ngauss), x, a.wid_max);
      }
    }
  }
  if (tid == 0) {
    sc[kGfChi2] = chi2;
    sc[kGfLambda] = lambda;
    sc[kGfNu] = nu;
  }
  if (!status) {
    if (tid == 0) {
      S.first = 0;
      S.nfev += 1;
      a.state[p] = S;
    }
    return;
  }

  // --- finished: parameters, covariance and errors at the current point
  __syncthreads();
  double* po = a.params + (size_t)p * npar;
  double* eo = a.perrs + (size_t)p * npar;
  double* co = a.cov ? a.cov + (size_t)p * npar * npar : nullptr;
  if (tid < npar) {
    const int kind = gf_kind<JOIN>(tid, npar, a.ngauss);
    const double x = st[kGfXi + tid];
    const double v = fl[tid] ? gf_to_ext(kind, x, a.wid_max) : a.pext[(size_t)p * npar + tid];
    po[tid] = v;
    a.pext[(size_t)p * npar + tid] = v;
    eo[tid] = 0.0;
    s_fac[tid] = gf_dext(kind, x, a.wid_max);
  }
  if (co)
    for (int e = tid; e < npar * npar; e += 256) co[e] = 0.0;
  for (int i = tid >> 4; i < nf; i += 16)
    for (int k = tid & 15; k <= i; k += 16) L[gf_tri(i, k)] = st[kGfHc + (size_t)i * nf + k];
  __syncthreads();
  const bool ok = nf > 0 && S.dof > 0 && status != PPF_GAUSS_NONFINITE && gf_cholesky(L, nf);
  __syncthreads();
  if (ok) {
    // column tid of the inverse: W[i][tid] in the trial-Hessian storage
    double* W = st + kGfHt;
    if (tid < nf) {
      const int t = tid;
      for (int i = 0; i < nf; ++i) {
        double s = i == t ? 1.0 : 0.0;
        for (int k = t; k < i; ++k) s -= L[gf_tri(i, k)] * W[(size_t)k * nf + t];
        W[(size_t)i * nf + t] = i < t ? 0.0 : s / L[gf_tri(i, i)];
      }
      for (int i = nf - 1; i >= 0; --i) {
        double s = W[(size_t)i * nf + t];
        for (int k = i + 1; k < nf; ++k) s -= L[gf_tri(k, i)] * W[(size_t)k * nf + t];
        W[(size_t)i * nf + t] = s / L[gf_tri(i, i)];
      }
    }
    __syncthreads();
    const double red = chi2 / (double)S.dof;  // lmfit's scale_covar
    for (int e = tid; e < nf * nf; e += 256) {
      const int i = e / nf, k = e % nf;
      const int qi = s_free[i], qk = s_free[k];
      const double c = W[(size_t)i * nf + k] * s_fac[qi] * s_fac[qk] * red;
      if (co) co[(size_t)qi * npar + qk] = c;
      if (i == k) eo[qi] = c > 0.0 ? sqrt(c) : 0.0;
    }
  }
  if (tid == 0) {
    a.chi2[p] = chi2;
    S.done = 1;
    S.status = status;
    S.first = 0;
    a.state[p] = S;
    int* info = a.info + 4 * p;
    info[0] = status;
    info[1] = S.nfev;
    info[2] = S.dof;
    info[3] = S.nfree;
  }
}

// The no-join kernels first and in the order they always had in the code
// object, then what the joint fits add.
template __global__ void k_gauss_basis<false>(GaussFitArgs);
template __global__ void k_gauss_gram<false>(GaussFitArgs);
template __global__ void k_gauss_init<false>(GaussFitArgs, const double*, const int*);
template __global__ void k_gauss_step<false>(GaussFitArgs, int);
template __global__ void k_gauss_basis<true>(GaussFitArgs);
template __global__ void k_gauss_gram<true>(GaussFitArgs);
template __global__ void k_gauss_init<true>(GaussFitArgs, const double*, const int*);
template __global__ void k_gauss_step<true>(GaussFitArgs, int);

// grid (ceil(nrow / 256)): *bad = 1 when a row's join group is outside
// 0 .. njoin - 1 (every writer stores the same value)
__global__ __launch_bounds__(256) void k_gauss_join_check(const int* __restrict__ join_of,
                                                          int64_t nrow, int njoin,
                                                          int* __restrict__ bad) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < nrow && (join_of[i] < 0 || join_of[i] >= njoin)) *bad = 1;
}

}  // namespace ppf
