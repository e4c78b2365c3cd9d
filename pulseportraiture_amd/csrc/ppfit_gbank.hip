// ppfit_gbank.hip -- the matched-filter bank of the automatic component
// search (pplib.auto_gaussian_profiles): for every profile p, width w and bin
// j the significance of the unit-amplitude Gaussian component of FWHM
// widths[w] centred on bin j in the residual of p.
//
// The template g is the component as the fit builds it (k_gauss_basis:
// bin-centre wrap, |z| < 20 support, rescale factor), scattered by 1 / (1 +
// 2 pi i k taun[p]).  With c = <resid, g> and gg = <g, g>,
//
//   amp = c / gg,   s2 = c^2 / (gg errs[p]^2) where c > 0, else 0.
//
// The template of bin j is the template of bin 0 turned by j bins, so c over
// all j is one circular correlation:
//
//   (k_rfft_rows      the residual spectra R, the existing row transform)
//   k_gauss_bank      one workgroup per (profile, width): the template of bin
//                     0 in LDS, its spectrum G, the scattering filter, gg by
//                     Parseval (DC and Nyquist weights as k_gauss_gram),
//                     irfft(R conj(G)) in LDS, the s2 map and a block argmax;
//   k_gauss_bank_best per profile, the maximum over the widths in width order.
//
// Ties go to the smaller width index, then to the smaller bin.  Every sum
// runs in a fixed order, a profile reads nothing of another profile: results
// are bitwise reproducible and independent of what else shares the call.  No
// atomics.
#include "ppfit_kernels.hpp"

namespace ppf {

constexpr int kBankMaxWid = 64;
struct GaussBankArgs {
  int nbin, nwid;
  double fwhm, sqrt2pi;         // 2 sqrt(2 ln 2), sqrt(2 pi) as numpy forms them
  double widths[kBankMaxWid];   // FWHM [rot]
  const double2* rspec;         // [nprof][nbin / 2 + 1] residual spectra
  const double* errs;           // [nprof]
  const double* taun;           // [nprof] tau / nbin
  const double2* tw;            // rfft twiddles of nbin
  double* s2;                   // [nprof][nwid][nbin] or null
  double* part;                 // [nprof][nwid][4]: s2, bin (-1: none), c, gg of the best bin
  double* best;                 // [nprof][4]: s2, loc, wid, amp
  int* best_idx;                // [nprof][2]: width index, bin
};

// grid (nwid, nprof)
template <int LOGN>
__global__ __launch_bounds__(kBlock) void k_gauss_bank(GaussBankArgs a) {
  constexpr int N = 1 << LOGN;  // complex points of the packed row
  constexpr int nbin = 2 * N;
  constexpr int KI = (N + 1 + kBlock - 1) / kBlock;
  constexpr int QB = (nbin + kBlock - 1) / kBlock;
  __shared__ double2 buf[N + 1];
  __shared__ double s_max[kWaves], s_red[kWaves];
  __shared__ int s_arg[kWaves];
  const int w = blockIdx.x, p = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int nwid = a.nwid;
  const double wid = a.widths[w];

  // --- the template of bin 0, as k_gauss_basis builds a component of amp 1
  const double start = 0.5 / (double)nbin, stop = 1.0 - 0.5 / (double)nbin;
  const double step = (stop - start) / (double)(nbin - 1);
  const double loc = start;  // bin centre 0
  const double sigma = wid / a.fwhm;
  const double mean = gf_py_mod1(loc);
  const double norm = __dmul_rn(sigma, a.sqrt2pi);
  double best = -1.0;
  int bi = nbin;
  double rv[QB];
#pragma unroll
  for (int q = 0; q < QB; ++q) {
    rv[q] = 0.0;
    const int j = tid + kBlock * q;
    if (j < nbin) {
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
  if (lane == 0) { s_max[wv] = best; s_arg[wv] = bi; }
  __syncthreads();
  double gb = s_max[0];
  int gi = s_arg[0];
  for (int v = 1; v < kWaves; ++v)
    if (s_max[v] > gb || (s_max[v] == gb && s_arg[v] < gi)) { gb = s_max[v]; gi = s_arg[v]; }
  __syncthreads();
  double fact = 1.0;
  const bool scale = gb != 0.0 && gi < nbin;
  if (scale) {
    const double z = (gf_locval(gi, nbin, start, stop, step, mean) - loc) / sigma;
    fact = exp(__dmul_rn(-0.5, __dmul_rn(z, z))) / gb;
  }
  double* row = reinterpret_cast<double*>(buf);  // buf[j] = (x_2j, x_2j+1)
#pragma unroll
  for (int q = 0; q < QB; ++q) {
    const int j = tid + kBlock * q;
    if (j < nbin) row[j] = scale ? __dmul_rn(fact, rv[q]) : rv[q];
  }
  __syncthreads();

  // --- its spectrum, scattered; gg by Parseval; R conj(G)
  lds_fft<LOGN, false>(buf, a.tw);
  const double2* R = a.rspec + (size_t)p * (N + 1);
  const double tn = a.taun[p];
  double2 xs[(N + kBlock) / kBlock + 1];
  double gsum = 0.0;
#pragma unroll
  for (int i = 0; i < KI; ++i) {
    const int k = tid + i * kBlock;
    if (k <= N) {
      double2 g = rfft_post<LOGN>(buf, k, a.tw);
      if (tn != 0.0) {  // S = 1 / (1 + 2 pi i k tau_n)
        const double ak = 2.0 * M_PI * (double)k * tn;
        const double den = 1.0 / (1.0 + ak * ak);
        g = cmul(cmk(den, -ak * den), g);
      }
      // the time-domain row keeps the real part at DC and Nyquist only
      const bool edge = k == 0 || k == N;
      if (edge) g.y = 0.0;
      gsum = fma(edge ? 1.0 : 2.0, fma(g.x, g.x, g.y * g.y), gsum);
      xs[i] = cmul(R[k], cconj(g));
    }
  }
  const double gg = block_sum(gsum, s_red) / (double)nbin;
  __syncthreads();

  // --- c = irfft(R conj(G)); the map and the best bin
  c2r_in_lds<LOGN>(buf, xs, a.tw);
  const double inv = 1.0 / (double)N;
  const double err = a.errs[p];
  const double den = gg * err * err;
  double2* map = a.s2 ? reinterpret_cast<double2*>(a.s2 + ((size_t)p * nwid + w) * nbin) : nullptr;
  double bv = 0.0;
  int bj = -1;
#pragma unroll
  for (int i = 0; i < KI; ++i) {
    const int j = tid + i * kBlock;
    if (j < N) {
      const double2 c = cscale(buf[j], inv);
      const double s0 = c.x > 0.0 ? c.x * c.x / den : 0.0;
      const double s1 = c.y > 0.0 ? c.y * c.y / den : 0.0;
      if (map) map[j] = cmk(s0, s1);
      if (s0 > bv) { bv = s0; bj = 2 * j; }
      if (s1 > bv) { bv = s1; bj = 2 * j + 1; }
    }
  }
  // (bv > 0 exactly when bj >= 0)
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const double ob = __shfl_xor(bv, o);
    const int oi = __shfl_xor(bj, o);
    if (ob > bv || (ob == bv && ob > 0.0 && oi < bj)) { bv = ob; bj = oi; }
  }
  if (lane == 0) { s_max[wv] = bv; s_arg[wv] = bj; }
  __syncthreads();
  if (tid == 0) {
    for (int v = 1; v < kWaves; ++v)
      if (s_max[v] > bv || (s_max[v] == bv && bv > 0.0 && s_arg[v] < bj)) {
        bv = s_max[v];
        bj = s_arg[v];
      }
    double* o = a.part + ((size_t)p * nwid + w) * 4;
    double c = 0.0;
    if (bj >= 0) {
      const double2 cc = buf[bj >> 1];
      c = ((bj & 1) ? cc.y : cc.x) * inv;
    }
    o[0] = bv;
    o[1] = (double)bj;
    o[2] = c;
    o[3] = gg;
  }
}

// one thread per profile
__global__ __launch_bounds__(64) void k_gauss_bank_best(GaussBankArgs a, int nprof) {
  const int p = blockIdx.x * 64 + threadIdx.x;
  if (p >= nprof) return;
  const int nbin = a.nbin;
  const double* part = a.part + (size_t)p * a.nwid * 4;
  double bv = 0.0;
  int bw = -1;
  for (int w = 0; w < a.nwid; ++w)
    if (part[4 * w] > bv && part[4 * w + 1] >= 0.0) { bv = part[4 * w]; bw = w; }
  double* o = a.best + (size_t)p * 4;
  int* oi = a.best_idx + (size_t)p * 2;
  if (bw < 0) {
    o[0] = o[1] = o[2] = o[3] = 0.0;
    oi[0] = oi[1] = -1;
    return;
  }
  const int j = (int)part[4 * bw + 1];
  const double start = 0.5 / (double)nbin, stop = 1.0 - 0.5 / (double)nbin;
  const double step = (stop - start) / (double)(nbin - 1);
  o[0] = bv;
  o[1] = (j == nbin - 1) ? stop : __dadd_rn(__dmul_rn((double)j, step), start);  // bin centre j
  o[2] = a.widths[bw];
  o[3] = part[4 * bw + 2] / part[4 * bw + 3];
  oi[0] = bw;
  oi[1] = j;
}

}  // namespace ppf
