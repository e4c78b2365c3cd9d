// ppfit_noisefit.hip -- the noise floor from a fit to the power spectrum
// (gfx950): get_noise_fit (pplib.py:2255-2287) and find_kc (pplib.py:1465-1495).
//
// find_kc fits model(k) = b f_a(k) + dc to d_k = log10(pows_k) by
// scipy.optimize.brute(Ns = 20, finish = None): the smallest weighted sum of
// squares over the 20 x 20 x 20 grid
//   a  = a_lo + ia (a_hi - a_lo) / 19   (1/n .. 1 for exp_dc, 1 .. n for half_tri)
//   b  = ib (max d - min d) / 19
//   dc = min d + idc (max d - min d) / 19
// with f_a(k) = e^{-a k} (exp_dc) or max(0, 1 - k / floor(a)) (half_tri).  The
// cutoff kc is the first k with e^{-a k} < 0.005 (n - 1 if none), or floor(a).
//
// One workgroup per spectrum.  The sum of squares is a quadratic in (b, dc):
// with d' = d - min d, dc' = dc - min d and, per a, the three sums
// Se = sum w f, See = sum w f^2, Sde = sum w d' f, beside Sw, Sd, Sdd,
//   S(a, b, dc) = [Sdd + dc' (dc' Sw - 2 Sd)] + b [b See + 2 (dc' Se - Sde)]
// so a row costs 20 n evaluations of f and 8,000 O(1) grid points, not
// 8,000 n.  The first bracket does not depend on a and the second is
// multiplied by b, so the b = 0 plane is bitwise the same for every a: a
// spectrum with no slope ties exactly there and the lowest flat index
// (ia = 0) wins, as numpy.argmin's first minimum does.  numpy.argmin also
// returns the first NaN: a spectrum holding a zero, negative or non-finite
// power (or a non-finite weight) makes the objective NaN at flat index 0 (b's
// step is inf or NaN there), so such a row returns index 0.
//
// Every reduction has a fixed order (thread t takes k = t, t + kBlock, ...;
// DPP wave sums; the four waves added in order) and nothing is shared between
// rows, so a row's outputs do not depend on what else is in the call.
#include "ppfit_kernels.hpp"

namespace ppf {

constexpr int kNfNs = 20;                       // brute's Ns
constexpr int kNfGrid = kNfNs * kNfNs * kNfNs;  // grid points per spectrum
constexpr double kNfFloor = 0.005;              // find_kc's e^{-a k} threshold

struct NoiseFitShared {
  double red[kWaves];
  double part[kNfNs][3][kWaves];  // per-wave Se, See, Sde of each a
  double tot[kNfNs][3];
  double bestv[kWaves];
  int besti[kWaves];
  int mink[kWaves];
};

// grid value i of brute's axis [lo, hi]: numpy.mgrid's i * ((hi - lo) / 19) + lo,
// each operation rounded on its own (floor(a) of half_tri depends on it)
__device__ __forceinline__ double nf_axis(double lo, double hi, int i) {
#pragma clang fp contract(off)
  const double step = (hi - lo) / (double)(kNfNs - 1);
  const double t = (double)i * step;
  return t + lo;
}

template <int FN>
__device__ __forceinline__ double nf_a(int n, int ia) {
  return FN == 0 ? nf_axis(1.0 / (double)n, 1.0, ia) : nf_axis(1.0, (double)n, ia);
}

template <int FN>
__device__ __forceinline__ double nf_basis(double a, int k) {
  if constexpr (FN == 0) {
    return exp(-a * (double)k);
  } else {
    const double fa = floor(a);
    return (double)k < fa ? 1.0 - (double)k / fa : 0.0;
  }
}

// numpy.argmin's order: the first NaN, else the smallest value, else the lower index
__device__ __forceinline__ bool nf_better(double v1, int i1, double v2, int i2) {
  const bool n1 = isnan(v1), n2 = isnan(v2);
  if (n1 || n2) return (n1 && n2) ? i1 < i2 : n1;
  if (v1 < v2) return true;
  if (v1 > v2) return false;
  return i1 < i2;
}

__device__ __forceinline__ double nf_block_max(double v, NoiseFitShared& sh) {
  v = wave_max(v);
  if ((threadIdx.x & 63) == 0) sh.red[threadIdx.x >> 6] = v;
  __syncthreads();
  double m = sh.red[0];
#pragma unroll
  for (int i = 1; i < kWaves; ++i) m = fmax(m, sh.red[i]);
  __syncthreads();
  return m;
}

// The grid search on d[0 .. n) (LDS; log10 of the powers), weights 1 / errs_k^2
// (errs in global memory, or NULL for 1).  Every thread returns the winner's
// flat index (ia * 20 + ib) * 20 + idc and kc.
template <int FN>
__device__ void nf_search(const double* d, const double* __restrict__ errs, int n,
                          NoiseFitShared& sh, int& idx_out, int& kc_out) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  // range of d; a d or weight that is not finite sends the row to index 0
  double mx = -INFINITY, mn = -INFINITY;
  int bad = 0;
  for (int k = tid; k < n; k += kBlock) {
    const double v = d[k];
    bad |= !isfinite(v);
    if (errs) {
      const double e = errs[k];
      bad |= !isfinite(1.0 / (e * e));
    }
    mx = fmax(mx, v);
    mn = fmax(mn, -v);
  }
  bad = __syncthreads_or(bad);
  int best = 0;
  if (!bad) {
    const double dmax = nf_block_max(mx, sh), dmin = -nf_block_max(mn, sh);
    double sw = 0.0, sd = 0.0, sdd = 0.0;
    for (int k = tid; k < n; k += kBlock) {
      double w = 1.0;
      if (errs) {
        const double e = errs[k];
        w = 1.0 / (e * e);
      }
      const double v = d[k] - dmin;
      sw += w;
      sd = fma(w, v, sd);
      sdd = fma(w * v, v, sdd);
    }
    sw = block_sum(sw, sh.red);
    sd = block_sum(sd, sh.red);
    sdd = block_sum(sdd, sh.red);
    for (int ia = 0; ia < kNfNs; ++ia) {
      const double a = nf_a<FN>(n, ia);
      double se = 0.0, see = 0.0, sde = 0.0;
      for (int k = tid; k < n; k += kBlock) {
        double w = 1.0;
        if (errs) {
          const double e = errs[k];
          w = 1.0 / (e * e);
        }
        const double f = nf_basis<FN>(a, k), wf = w * f;
        se += wf;
        see = fma(wf, f, see);
        sde = fma(wf, d[k] - dmin, sde);
      }
      se = wave_sum(se);
      see = wave_sum(see);
      sde = wave_sum(sde);
      if (lane == 0) {
        sh.part[ia][0][wv] = se;
        sh.part[ia][1][wv] = see;
        sh.part[ia][2][wv] = sde;
      }
    }
    __syncthreads();
    if (tid < kNfNs * 3) {
      const double* p = &sh.part[0][0][0] + tid * kWaves;
      double s = 0.0;
#pragma unroll
      for (int i = 0; i < kWaves; ++i) s += p[i];
      (&sh.tot[0][0])[tid] = s;
    }
    __syncthreads();
    const double step = (dmax - dmin) / (double)(kNfNs - 1);
    double bv = INFINITY;
    int bi = kNfGrid;
    for (int g = tid; g < kNfGrid; g += kBlock) {
      const int ia = g / (kNfNs * kNfNs), ib = (g / kNfNs) % kNfNs, idc = g % kNfNs;
      const double b = (double)ib * step, dc = (double)idc * step;
      const double q0 = sdd + dc * (dc * sw - 2.0 * sd);
      const double q1 = b * sh.tot[ia][1] + 2.0 * (dc * sh.tot[ia][0] - sh.tot[ia][2]);
      const double v = fma(b, q1, q0);
      if (nf_better(v, g, bv, bi)) { bv = v; bi = g; }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      const double ov = __shfl_xor(bv, o);
      const int oi = __shfl_xor(bi, o);
      if (nf_better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
    }
    if (lane == 0) { sh.bestv[wv] = bv; sh.besti[wv] = bi; }
    __syncthreads();
    bv = sh.bestv[0];
    bi = sh.besti[0];
#pragma unroll
    for (int i = 1; i < kWaves; ++i)
      if (nf_better(sh.bestv[i], sh.besti[i], bv, bi)) { bv = sh.bestv[i]; bi = sh.besti[i]; }
    best = bi;
  }
  const double a = nf_a<FN>(n, best / (kNfNs * kNfNs));
  int kc;
  if constexpr (FN == 0) {
    int mk = n - 1;
    for (int k = tid; k < n; k += kBlock)
      if (exp(-a * (double)k) < kNfFloor) { mk = min(mk, k); break; }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) mk = min(mk, __shfl_xor(mk, o));
    __syncthreads();  // sh.besti has been read by every thread
    if (lane == 0) sh.mink[wv] = mk;
    __syncthreads();
    kc = sh.mink[0];
#pragma unroll
    for (int i = 1; i < kWaves; ++i) kc = min(kc, sh.mink[i]);
  } else {
    kc = (int)floor(a);
  }
  __syncthreads();
  idx_out = best;
  kc_out = kc;
}

// get_noise_fit's tail (pplib.py:2273-2277) on pows[0 .. NH) (LDS)
__device__ __forceinline__ void nf_finish(const double* pows, int NH, int kc, int idx,
                                          double fact, NoiseFitShared& sh, int r,
                                          double* __restrict__ noise, int* __restrict__ kc_out,
                                          int* __restrict__ idx_out) {
  double k_crit = fact * (double)kc;
  if (k_crit >= (double)NH) k_crit = fmin((double)(int)(0.99 * (double)NH), k_crit);
  const int k0 = (int)k_crit;
  double p = 0.0;
  for (int k = k0 + threadIdx.x; k < NH; k += kBlock) p += pows[k];
  p = block_sum(p, sh.red);
  if (threadIdx.x == 0) {
    noise[r] = sqrt(p / (double)(NH - k0));
    if (kc_out) kc_out[r] = kc;
    if (idx_out) idx_out[r] = idx;
  }
}

// get_noise_fit per row.  The row's LDS buffer is reused: once every thread
// holds its powers in registers, pows[NH] and d[NH] take the place of the
// row (2 NH doubles: kLdsSpec).
template <class Row>
__global__ __launch_bounds__(kBlock) void k_noise_fit_rows(const double* __restrict__ in,
                                                           double fact,
                                                           double* __restrict__ noise,
                                                           int* __restrict__ kc_out,
                                                           int* __restrict__ idx_out,
                                                           const double2* __restrict__ tw,
                                                           Row row) {
  constexpr int KI = Row::kMaxKI;
  __shared__ typename Row::template Lds<kLdsSpec> sm;
  __shared__ NoiseFitShared sh;
  typename Row::Dev t(row, sm, tw);
  const int r = blockIdx.x, nbin = t.nbin(), NH = t.nh();
  t.load(in + (size_t)r * nbin);
  double pv[KI];
#pragma unroll
  for (int i = 0; i < KI; ++i) {
    const int k = threadIdx.x + i * kBlock;
    pv[i] = k < NH ? cabs2(t.bin(k)) / (double)nbin : 0.0;
  }
  t.release();
  double* pows = t.reals();
  double* d = pows + NH;
#pragma unroll
  for (int i = 0; i < KI; ++i) {
    const int k = threadIdx.x + i * kBlock;
    if (k < NH) {
      pows[k] = pv[i];
      d[k] = log10(pv[i]);
    }
  }
  __syncthreads();
  int idx, kc;
  nf_search<0>(d, nullptr, NH, sh, idx, kc);
  nf_finish(pows, NH, kc, idx, fact, sh, r, noise, kc_out, idx_out);
}

// find_kc on given power spectra pows [nrow][n], n in [4, 8193]; errs [n] or
// NULL.  Dynamic LDS: n doubles.
template <int FN>
__global__ __launch_bounds__(kBlock) void k_find_kc_rows(const double* __restrict__ pows,
                                                         const double* __restrict__ errs, int n,
                                                         int* __restrict__ kc_out,
                                                         int* __restrict__ idx_out) {
  extern __shared__ __align__(16) unsigned char gsm[];
  double* d = reinterpret_cast<double*>(gsm);
  __shared__ NoiseFitShared sh;
  const int r = blockIdx.x;
  for (int k = threadIdx.x; k < n; k += kBlock) d[k] = log10(pows[(size_t)r * n + k]);
  __syncthreads();
  int idx, kc;
  nf_search<FN>(d, errs, n, sh, idx, kc);
  if (threadIdx.x == 0) {
    kc_out[r] = kc;
    if (idx_out) idx_out[r] = idx;
  }
}

#define PPF_INST_NF(R)                                                                  \
  template __global__ void k_noise_fit_rows<R>(const double*, double, double*, int*, int*, \
                                               const double2*, R);
PPF_INST_NF(RowPow2<5>)
PPF_INST_NF(RowPow2<6>)
PPF_INST_NF(RowPow2<7>)
PPF_INST_NF(RowPow2<8>)
PPF_INST_NF(RowPow2<9>)
PPF_INST_NF(RowPow2<10>)
PPF_INST_NF(RowPow2<11>)
PPF_INST_NF(RowPow2<12>)
PPF_INST_NF(RowAny)
PPF_INST_NF(RowSmooth<1024>)
PPF_INST_NF(RowSmooth<4096>)
template __global__ void k_find_kc_rows<0>(const double*, const double*, int, int*, int*);
template __global__ void k_find_kc_rows<1>(const double*, const double*, int, int*, int*);

}  // namespace ppf
