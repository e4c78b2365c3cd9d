// ppfit_swt.hip -- wavelet smoothing of profiles on the device: pplib's
// wavelet_smooth, fit_wavelet_smooth_function and smart_smooth
// (pplib.py:1621-1761), built from the definition of the transform, not from
// PyWavelets' code.
//
// The transform is the undecimated (stationary) db8 transform with periodic
// extension.  h = kSwtH is the scaling filter in PyWavelets' rec_lo order,
// g[k] = (-1)^k h[15 - k]; with N = nbin, s_j = 2^(j-1) and a_0 the profile,
//   a_j[n] = sum_k h[k] a_{j-1}[(n + s_j k) mod N]
//   d_j[n] = sum_k g[k] a_{j-1}[(n + s_j k) mod N]            j = 1 .. L
//   lambda = fact median(|a_L u d_L|) / 0.6745 sqrt(2 ln N)
//   a_{j-1}[n] = 1/2 sum_k (h[k] a_j[(n - s_j k) mod N]
//                           + g[k] T(d_j)[(n - s_j k) mod N])  j = L .. 1
// from T(a_L), T the hard (c -> 0 where |c| < lambda) or soft (c ->
// sign(c) max(|c| - lambda, 0)) threshold.  The approximation is thresholded
// too and the median is that of the deepest pair, as in the reference.
//
//   k_swt_forward    one workgroup per row, the row ping-ponged in LDS: every
//                    d_j and a_j up to the row's deepest level into the
//                    workspace W[row][level][d, a][nbin]; whether the row has
//                    a non-zero sample;
//   k_swt_median     per (level, row): the exact median of the 2 N magnitudes
//                    of (a_j, d_j), a radix select on their bit patterns;
//   k_swt_objective  fit_wavelet_smooth_function at one (row, level, fact):
//                    the 30 grid points of every (row, level) of a search as
//                    independent workgroups, or one given point per row;
//   k_swt_polish     per (row, level): scipy's fmin (nm_polish) from the first
//                    grid minimum, each evaluation the same device function;
//   k_swt_smooth     per row: the smoothed row at a given (level, fact), or at
//                    the search's argmin over levels with the reduced chi^2
//                    and the zeroing of smart_smooth.
//
// An evaluation thresholds a_L into LDS, runs the inverse through two LDS rows
// reading the d_j from the workspace, and reduces: sum ((prof - s) / noise)^2,
// the signal sum_{k>=1} |S_k|^2 = (N sum s^2 - S_0^2 + S_{N/2}^2) / 2 (no
// transform), and get_noise_PS of s -- the LDS FFT for the powers of two from
// 64 up, direct sums of the top-quarter harmonics (dft_bin) otherwise.
//
// Every sum runs in a fixed order (a thread's strided partial, then
// block_sum), the only atomics are integer counts of the radix select, and a
// row's launches read no other row: the results are bitwise reproducible and
// independent of what else shares the call.
#include "ppfit_kernels.hpp"

namespace ppf {

// db8 scaling filter (rec_lo order): the minimum-phase spectral factor of the
// Daubechies polynomial, derived in 60-digit arithmetic
__device__ __constant__ double kSwtH[16] = {
    0.054415842243104008,   0.31287159091429995,     0.67563073629728976,
    0.58535468365420673,    -0.015829105256349306,   -0.28401554296154691,
    0.00047248457391328279, 0.12874742662047847,     -0.017369301001807547,
    -0.044088253930794755,  0.013981027917398282,    0.0087460940474057766,
    -0.0048703529934515741, -0.00039174037337694705, 0.00067544940645056933,
    -0.00011747678412476953};

constexpr int kSwtTaps = 16;
constexpr int kSwtGrid = 30;       // opt.brute's Ns on (0, 3)
constexpr double kSwtHi = 3.0;

struct SwtArgs {
  int nbin, L;            // L: levels the workspace holds per row
  int soft;               // threshold: 0 hard, 1 soft
  int kc;                 // first harmonic of get_noise_PS's top quarter
  double tol;             // rchi2_tol
  double sq2ln;           // sqrt(2 ln nbin) (host libm)
  const double* rows;     // [nrow][nbin]
  const int* nlev;        // [nrow] levels per row, or null: L
  const double* fact;     // [nrow] (given points) or null
  double* W;              // [nrow][L][2][nbin]: d_j, a_j
  double* med;            // [nrow][L] median |a_j u d_j|
  int* nz;                // [nrow] the row has a non-zero sample
  const double* noise;    // [nrow] get_noise_PS of the rows
  double* fgrid;          // [nrow][L][kSwtGrid] grid objectives
  double* pfact;          // [nrow][L] polished fact
  double* pfun;           // [nrow][L] and objective
  const double2* tw;      // rfft twiddles of nbin
  double* out;            // [nrow][nbin] smoothed rows
  double* o_obj;          // [nrow] objective (given points)
  double* o_rchi2;        // [nrow]
  int* o_nlevel;          // [nrow] (search)
  double* o_fact;         // [nrow] (search)
  int* o_zeroed;          // [nrow] (search)
};

__device__ __forceinline__ double swt_g(int k) {
  return (k & 1) ? -kSwtH[kSwtTaps - 1 - k] : kSwtH[kSwtTaps - 1 - k];
}

__device__ __forceinline__ double swt_thresh(double c, double lam, int soft) {
  const double m = fabs(c);
  if (soft) {
    const double r = fmax(m - lam, 0.0);
    return c > 0.0 ? r : (c < 0.0 ? -r : 0.0);
  }
  return m < lam ? 0.0 : c;
}

__device__ __forceinline__ const double* swt_d(const SwtArgs& a, int r, int j) {
  return a.W + (((size_t)r * a.L + (j - 1)) * 2) * a.nbin;
}
__device__ __forceinline__ const double* swt_a(const SwtArgs& a, int r, int j) {
  return swt_d(a, r, j) + a.nbin;
}

// lambda of (row, level) at fact, in the reference's order of operations
__device__ __forceinline__ double swt_lambda(const SwtArgs& a, int r, int lev, double fact) {
  const double med = a.med[(size_t)r * a.L + (lev - 1)];
  return __dmul_rn(__dmul_rn(fact, __ddiv_rn(med, 0.6745)), a.sq2ln);
}

// grid (nrow), 2 nbin doubles of dynamic LDS
__global__ __launch_bounds__(kBlock) void k_swt_forward(SwtArgs a) {
  extern __shared__ __align__(16) unsigned char swt_lds[];
  const int r = blockIdx.x, N = a.nbin, tid = threadIdx.x;
  const int L = a.nlev ? a.nlev[r] : a.L;
  double* cur = reinterpret_cast<double*>(swt_lds);
  double* nxt = cur + N;
  const double* x = a.rows + (size_t)r * N;
  int any = 0;
  for (int n = tid; n < N; n += kBlock) {
    const double v = x[n];
    cur[n] = v;
    any |= (v != 0.0);  // (a NaN counts as a sample, as in np.any)
  }
  any = __syncthreads_or(any);
  if (tid == 0) a.nz[r] = any;
  for (int j = 1; j <= L; ++j) {
    const int s = 1 << (j - 1);
    double* dj = a.W + (((size_t)r * a.L + (j - 1)) * 2) * N;
    double* aj = dj + N;
    int off[kSwtTaps];  // the dilated filter may wrap many times
#pragma unroll
    for (int k = 0; k < kSwtTaps; ++k) off[k] = (s * k) % N;
    for (int n = tid; n < N; n += kBlock) {
      double sa = 0.0, sd = 0.0;
#pragma unroll
      for (int k = 0; k < kSwtTaps; ++k) {
        int i = n + off[k];
        if (i >= N) i -= N;
        const double v = cur[i];
        sa = fma(kSwtH[k], v, sa);
        sd = fma(swt_g(k), v, sd);
      }
      nxt[n] = sa;
      aj[n] = sa;
      dj[n] = sd;
    }
    __syncthreads();
    double* t = cur; cur = nxt; nxt = t;
  }
}

// The k-th smallest (0-based) of the bit patterns of |v[0 .. n)| (non-negative
// doubles order as their patterns): eight passes of an 8-bit histogram over
// the values that share the prefix found so far.  Every thread returns it.
__device__ inline unsigned long long swt_select(const double* __restrict__ v, int n, int k,
                                                int* hist) {
  unsigned long long prefix = 0ull;
  for (int p = 7; p >= 0; --p) {
    const int shift = 8 * p;
    hist[threadIdx.x] = 0;  // kBlock == 256 bins
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += kBlock) {
      const unsigned long long key = (unsigned long long)__double_as_longlong(fabs(v[i]));
      const bool in = p == 7 || (key >> (shift + 8)) == (prefix >> (shift + 8));
      if (in) atomicAdd(&hist[(int)((key >> shift) & 255ull)], 1);
    }
    __syncthreads();
    int cum = 0, b = 0;
    for (; b < 255; ++b) {
      const int c = hist[b];
      if (cum + c > k) break;
      cum += c;
    }
    k -= cum;
    prefix |= (unsigned long long)b << shift;
    __syncthreads();
  }
  return prefix;
}

// grid (L, nrow): numpy's median (the mean of the two middle order
// statistics) of the 2 N magnitudes of level blockIdx.x + 1; deepest: only
// the row's deepest level
__global__ __launch_bounds__(kBlock) void k_swt_median(SwtArgs a, int deepest) {
  __shared__ int hist[kBlock];
  const int j = blockIdx.x + 1, r = blockIdx.y;
  const int L = a.nlev ? a.nlev[r] : a.L;
  if (deepest ? j != L : j > L) return;
  const double* v = swt_d(a, r, j);  // d_j then a_j: 2 N contiguous values
  const int n = 2 * a.nbin;
  const unsigned long long lo = swt_select(v, n, n / 2 - 1, hist);
  const unsigned long long hi = swt_select(v, n, n / 2, hist);
  if (threadIdx.x == 0)
    a.med[(size_t)r * a.L + (j - 1)] =
        (__longlong_as_double((long long)lo) + __longlong_as_double((long long)hi)) / 2.0;
}

// The smoothed row of (r, lev) at threshold lam, through the LDS rows b0, b1;
// returns the one that holds it (all threads past a barrier).
__device__ inline double* swt_inverse(const SwtArgs& a, int r, int lev, double lam, double* b0,
                                      double* b1) {
  const int N = a.nbin, tid = threadIdx.x;
  const double* aL = swt_a(a, r, lev);
  for (int n = tid; n < N; n += kBlock) b0[n] = swt_thresh(aL[n], lam, a.soft);
  __syncthreads();
  double* cur = b0;
  double* nxt = b1;
  for (int j = lev; j >= 1; --j) {
    const int s = 1 << (j - 1);
    const double* dj = swt_d(a, r, j);
    int off[kSwtTaps];
#pragma unroll
    for (int k = 0; k < kSwtTaps; ++k) off[k] = (s * k) % N;
    for (int n = tid; n < N; n += kBlock) {
      double acc = 0.0;
#pragma unroll
      for (int k = 0; k < kSwtTaps; ++k) {
        int i = n - off[k];
        if (i < 0) i += N;
        acc = fma(kSwtH[k], cur[i], acc);
        acc = fma(swt_g(k), swt_thresh(dj[i], lam, a.soft), acc);
      }
      nxt[n] = 0.5 * acc;
    }
    __syncthreads();
    double* t = cur; cur = nxt; nxt = t;
  }
  return cur;
}

// sum ((prof - s) / noise)^2 / N (get_red_chi2, pplib.py:727-750, dof = N)
__device__ __forceinline__ double swt_rchi2(const SwtArgs& a, int r, const double* s, double* red) {
  const int N = a.nbin;
  const double* x = a.rows + (size_t)r * N;
  const double err = a.noise[r];
  double c = 0.0;
  for (int n = threadIdx.x; n < N; n += kBlock) {
    const double q = (x[n] - s[n]) / err;
    c = fma(q, q, c);
  }
  return block_sum(c, red) / (double)N;
}

// fit_wavelet_smooth_function (pplib.py:1737-1761) of the smoothed row s
// (LDS; other: the second LDS row, overwritten).  LOGN = log2(nbin / 2) for
// the FFT kernels' lengths, 0: any nbin.
template <int LOGN>
__device__ inline double swt_objective(const SwtArgs& a, int r, const double* s, double* other,
                                       double* red, double& rchi2) {
  const int N = a.nbin, tid = threadIdx.x, NH = N / 2 + 1;
  double ss = 0.0, s0 = 0.0, sn = 0.0;
  for (int n = tid; n < N; n += kBlock) {
    const double v = s[n];
    ss = fma(v, v, ss);
    s0 += v;
    sn += (n & 1) ? -v : v;
  }
  rchi2 = swt_rchi2(a, r, s, red);
  ss = block_sum(ss, red);
  s0 = block_sum(s0, red);
  sn = block_sum(sn, red);
  const double signal = 0.5 * ((double)N * ss - s0 * s0 + sn * sn);
  double p = 0.0;
  if constexpr (LOGN > 0) {
    constexpr int H = 1 << LOGN;
    double2* buf = reinterpret_cast<double2*>(other);
    for (int n = tid; n < N; n += kBlock) other[n] = s[n];
    __syncthreads();
    lds_fft<LOGN, false>(buf, a.tw);
    for (int k = a.kc + tid; k <= H; k += kBlock) p += cabs2(rfft_post<LOGN>(buf, k, a.tw));
  } else {
    for (int k = a.kc + tid; k < NH; k += kBlock) p += cabs2(dft_bin(s, N, k, a.tw));
  }
  p = block_sum(p, red);
  const double noise = sqrt(p / (double)N / (double)(NH - a.kc)) * sqrt((double)N / 2.0);
  double snr = 0.0;
  if (signal != 0.0) snr = noise != 0.0 ? signal / noise : INFINITY;
  if (fabs(rchi2 - 1.0) > a.tol) snr = 0.0;
  return -snr;
}

__device__ __forceinline__ double swt_grid_fact(int g) {
  return __dmul_rn((double)g, kSwtHi / (double)(kSwtGrid - 1));  // np.mgrid[0:3:30j]
}

// given == 0: grid (kSwtGrid, L, nrow), the search's grid; given == 1: grid
// (1, 1, nrow), each row at its (nlev, fact).  2 nbin doubles of dynamic LDS.
template <int LOGN>
__global__ __launch_bounds__(kBlock) void k_swt_objective(SwtArgs a, int given) {
  extern __shared__ __align__(16) unsigned char swt_lds[];
  __shared__ double red[kWaves];
  double* b0 = reinterpret_cast<double*>(swt_lds);
  double* b1 = b0 + a.nbin;
  const int r = blockIdx.z;
  const int lev = given ? a.nlev[r] : (int)blockIdx.y + 1;
  const double fact = given ? a.fact[r] : swt_grid_fact(blockIdx.x);
  if (!given && !a.nz[r]) return;
  double* s = swt_inverse(a, r, lev, swt_lambda(a, r, lev, fact), b0, b1);
  double rc;
  const double f = swt_objective<LOGN>(a, r, s, s == b0 ? b1 : b0, red, rc);
  if (threadIdx.x == 0) {
    if (given) {
      a.o_obj[r] = f;
      a.o_rchi2[r] = rc;
    } else {
      a.fgrid[((size_t)r * a.L + (lev - 1)) * kSwtGrid + blockIdx.x] = f;
    }
  }
}

// grid (L, nrow): opt.brute's finish, scipy's fmin from the first grid minimum
template <int LOGN>
__global__ __launch_bounds__(kBlock) void k_swt_polish(SwtArgs a) {
  extern __shared__ __align__(16) unsigned char swt_lds[];
  __shared__ double red[kWaves];
  double* b0 = reinterpret_cast<double*>(swt_lds);
  double* b1 = b0 + a.nbin;
  const int lev = blockIdx.x + 1, r = blockIdx.y;
  if (!a.nz[r]) return;
  const double* fg = a.fgrid + ((size_t)r * a.L + (lev - 1)) * kSwtGrid;
  double bv = NAN;
  int bi = 0x7fffffff;
  for (int g = 0; g < kSwtGrid; ++g) {
    const double v = fg[g];
    if (argmin_better(v, g, bv, bi)) { bv = v; bi = g; }
  }
  const int maxfun = 200;
  int fcalls = 0;
  bool stop = false;
  auto F = [&](double xv) -> double {
    if (fcalls >= maxfun) { stop = true; return 0.0; }
    ++fcalls;
    double* s = swt_inverse(a, r, lev, swt_lambda(a, r, lev, xv), b0, b1);
    double rc;
    return swt_objective<LOGN>(a, r, s, s == b0 ? b1 : b0, red, rc);
  };
  double s0, f0, s1, f1;
  nm_polish(F, stop, fcalls, maxfun, swt_grid_fact(bi), s0, f0, s1, f1);
  if (threadIdx.x == 0) {
    a.pfact[(size_t)r * a.L + (lev - 1)] = s0;
    a.pfun[(size_t)r * a.L + (lev - 1)] = fmin(f0, f1);
  }
}

// grid (nrow), 2 nbin doubles of dynamic LDS.  pick == 0: out[r] = the row
// smoothed at its (nlev, fact).  pick == 1: at the argmin over levels of the
// polished objectives (the first on ties), zeroed when the reduced chi^2 is
// further than tol from 1; an all-zero row stays zero (level 0).
__global__ __launch_bounds__(kBlock) void k_swt_smooth(SwtArgs a, int pick) {
  extern __shared__ __align__(16) unsigned char swt_lds[];
  __shared__ double red[kWaves];
  double* b0 = reinterpret_cast<double*>(swt_lds);
  double* b1 = b0 + a.nbin;
  const int r = blockIdx.x, N = a.nbin, tid = threadIdx.x;
  double* out = a.out + (size_t)r * N;
  int lev;
  double fact;
  if (pick) {
    if (!a.nz[r]) {
      for (int n = tid; n < N; n += kBlock) out[n] = 0.0;
      if (tid == 0) {
        a.o_nlevel[r] = 0;
        a.o_fact[r] = 0.0;
        a.o_rchi2[r] = 0.0;
        a.o_zeroed[r] = 0;
      }
      return;
    }
    double bv = NAN;
    int bi = 0x7fffffff;
    for (int j = 0; j < a.L; ++j) {
      const double v = a.pfun[(size_t)r * a.L + j];
      if (argmin_better(v, j, bv, bi)) { bv = v; bi = j; }
    }
    lev = bi + 1;
    fact = a.pfact[(size_t)r * a.L + bi];
  } else {
    lev = a.nlev[r];
    fact = a.fact[r];
  }
  const double* s = swt_inverse(a, r, lev, swt_lambda(a, r, lev, fact), b0, b1);
  if (!pick) {
    for (int n = tid; n < N; n += kBlock) out[n] = s[n];
    return;
  }
  const double rc = swt_rchi2(a, r, s, red);
  const bool zero = fabs(rc - 1.0) > a.tol;
  for (int n = tid; n < N; n += kBlock) out[n] = zero ? 0.0 : s[n];
  if (tid == 0) {
    a.o_nlevel[r] = lev;
    a.o_fact[r] = fact;
    a.o_rchi2[r] = rc;
    a.o_zeroed[r] = zero ? 1 : 0;
  }
}

}  // namespace ppf
