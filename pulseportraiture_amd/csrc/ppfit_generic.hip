// ppfit_generic.hip -- the fit's data pass for any nbin (gfx950).
//
// The reference transforms profiles with numpy's rfft / irfft of whatever
// length the archive has (pptoaslib.py:976-978, pplib.py:2338-2426).  The
// register and LDS FFTs of ppfit_spectra.hip are built per power of two; for
// every other nbin in [16, 8192] the row kernels (template spectra, row
// rotations, FFTFIT, noise rows, irfft, zapping residuals, ppalign's
// rotate-and-sum, the generators) are the same bodies instantiated with
// RowAny (ppfit_rowfft.hpp): direct sums, O(nbin^2) per row instead of
// O(nbin log nbin).  What has no power-of-two twin is here: the fit's data
// pass forms all bins D_k = sum_m x_m e^{-2 pi i m k / nbin} of a chunk as a
// GEMM on the fp64 matrix cores against the twiddle table (k_dft_rows_mfma),
// and k_data_post_gen turns them into the fit's inputs.  An even nbin with
// nbin / 2 = 2^a 3^b 5^c has a mixed-radix FFT (RowSmooth): there
// k_data_fft_rows takes the GEMM's place, into the same rows.
#include "ppfit_kernels.hpp"

namespace ppf {

// ---------------------------------------------------------------------------
// The data pass's transforms on the fp64 matrix cores: D = rfft of every row
// of the chunk as two GEMMs over the pair index m' = 1 .. M = (nbin - 1) / 2,
//   Re D_k = x_0 + [even] (-1)^k x_{nbin/2} + sum_m' (x_m' + x_{nbin-m'}) cos(2 pi m' k / nbin)
//   Im D_k =                                sum_m' (x_m' - x_{nbin-m'}) (-sin)(2 pi m' k / nbin)
// (dft_bin's sums, ppfit_rowfft.hpp, with every cos / sin an exact table value tw[(m' k) mod
// nbin] instead of a phasor chain).  Workgroup: 16 kGenRT rows x 256 bins,
// wave w the bins k0 + 64 w .. + 63 as four 16 x 16 tiles per row tile; per step of 4 pair
// indices one v_mfma_f64_16x16x4 per tile and part, A = the 16 rows' pair
// sums (lane l: row l & 15, m' = m0 + (l >> 4)), B = the table values
// (lane l: m' = m0 + (l >> 4), bin l & 15 of the tile).  Output: D into the
// X rows (k < nbin/2 + 1); k_data_post_gen turns them into X in place.
// ---------------------------------------------------------------------------
typedef double gen_f64x4 __attribute__((ext_vector_type(4)));
constexpr int kGenLdsTw = 4096;  // 64 KB of LDS

// LTW: the twiddle table staged in LDS (nbin <= kGenLdsTw), else read from L2.
// Each workgroup takes kGenRT tiles of 16 rows, so every table value a lane
// gathers feeds kGenRT MFMAs per part; the rows' pair sums go through LDS in
// chunks of kGenChunk pair indices, loaded coalesced (16 threads per row
// segment) by the whole workgroup.
#ifndef PPF_DFT_RT
#define PPF_DFT_RT 2  // A/B knob: row tiles per workgroup
#endif
constexpr int kGenChunk = 64;
constexpr int kGenRT = PPF_DFT_RT;
constexpr int kGenRows = 16 * kGenRT;
inline size_t dft_mfma_lds(int nbin, bool ltw) {
  return (ltw ? (size_t)nbin * sizeof(double2) : 0) +
         2 * (size_t)kGenChunk * kGenRows * sizeof(double);
}
template <bool LTW>
__global__ __launch_bounds__(kBlock) void k_dft_rows_mfma(const double* __restrict__ rows,
                                                          double2* __restrict__ D, int nrows,
                                                          int nbin, int NHP,
                                                          const double2* __restrict__ twg) {
  extern __shared__ __align__(16) unsigned char gsm[];
  const double2* tw = twg;
  double* sp_l = reinterpret_cast<double*>(gsm + (LTW ? (size_t)nbin * sizeof(double2) : 0));
  double* sm_l = sp_l + kGenChunk * kGenRows;
  if constexpr (LTW) {
    double2* t = reinterpret_cast<double2*>(gsm);
    for (int i = threadIdx.x; i < nbin; i += kBlock) t[i] = twg[i];
    tw = t;  // published by the chunk loop's first barrier
  }
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int row0 = blockIdx.x * kGenRows, k0 = blockIdx.y * 256 + w * 64;
  const int NH = nbin / 2 + 1, M = (nbin - 1) / 2;
  const bool active = k0 < NH;  // wave-uniform: the wave has bins to compute
  const int ri = lane & 15, kk = lane >> 4;
  // the chunk loader: thread t fills pair indices 4 (t & 15) .. + 3 of rows
  // (t >> 4) + 16 q, q < kGenRT
  const int lr = tid >> 4, lq = tid & 15;
  // per tile j: the lane's bin and the table index (m' k) mod nbin at m' = 1 + kk
  int kj[4], idx[4], stp[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int k = k0 + 16 * j + ri;
    kj[j] = k < NH ? k : 0;  // bins past the end compute bin 0, never stored
    idx[j] = (int)(((long long)(1 + kk) * kj[j]) % nbin);
    stp[j] = (int)((4LL * kj[j]) % nbin);
  }
  gen_f64x4 cre[kGenRT][4], cim[kGenRT][4];
#pragma unroll
  for (int q = 0; q < kGenRT; ++q)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      cre[q][j] = (gen_f64x4){0.0, 0.0, 0.0, 0.0};
      cim[q][j] = cre[q][j];
    }
  for (int c0 = 1; c0 <= M; c0 += kGenChunk) {
    __syncthreads();  // the previous chunk has been consumed
#pragma unroll
    for (int q = 0; q < kGenRT; ++q) {
      const int lrow = lr + 16 * q;
      const bool ok = row0 + lrow < nrows;
      const double* xl = rows + (size_t)(ok ? row0 + lrow : 0) * nbin;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int mm = 4 * lq + i, m = c0 + mm;
        double a = 0.0, b = 0.0;
        if (ok && m <= M) {
          a = xl[m];
          b = xl[nbin - m];
        }
        sp_l[mm * kGenRows + lrow] = a + b;
        sm_l[mm * kGenRows + lrow] = a - b;
      }
    }
    __syncthreads();
    if (active) {
      const int nst = min(kGenChunk / 4, (M - c0) / 4 + 1);  // steps with any m' <= M
      for (int st = 0; st < nst; ++st) {
        double sp[kGenRT], sm[kGenRT];
#pragma unroll
        for (int q = 0; q < kGenRT; ++q) {
          sp[q] = sp_l[(4 * st + kk) * kGenRows + 16 * q + ri];
          sm[q] = sm_l[(4 * st + kk) * kGenRows + 16 * q + ri];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const double2 t = tw[idx[j]];
#pragma unroll
          for (int q = 0; q < kGenRT; ++q) {
            cre[q][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(sp[q], t.x, cre[q][j], 0, 0, 0);
            cim[q][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(sm[q], t.y, cim[q][j], 0, 0, 0);
          }
          idx[j] += stp[j];
          if (idx[j] >= nbin) idx[j] -= nbin;
        }
      }
    }
  }
  if (!active) return;
  // lane l holds rows (l >> 4) + 4 r of each row tile, bin l & 15 of each bin tile
#pragma unroll
  for (int q = 0; q < kGenRT; ++q)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = row0 + 16 * q + kk + 4 * r;
      if (row >= nrows) continue;
      const double* xo = rows + (size_t)row * nbin;
      const double x0 = xo[0], xn = (nbin & 1) ? 0.0 : xo[nbin / 2];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int k = k0 + 16 * j + ri;
        if (k < NH) {
          const double re = cre[q][j][r] + x0 + ((k & 1) ? -xn : xn);
          D[(size_t)row * NHP + k] = cmk(re, cim[q][j][r]);
        }
      }
    }
}

// The same spectra for a length with a mixed-radix FFT (RowSmooth): one
// workgroup per row, bins k < nbin/2 + 1 into row r of D (stride NHP).
template <class Row>
__global__ __launch_bounds__(kBlock) void k_data_fft_rows(const double* __restrict__ rows,
                                                          double2* __restrict__ D, int NHP,
                                                          const double2* __restrict__ tw, Row row) {
  __shared__ typename Row::template Lds<kLdsRow> sm;
  typename Row::Dev t(row, sm, tw);
  const size_t r = blockIdx.x;
  const int NH = t.nh();
  t.load(rows + r * t.nbin());
  for (int k = threadIdx.x; k < NH; k += kBlock) D[r * NHP + k] = t.bin(k);
}
#define PPF_INST_DATA_FFT(R) \
  template __global__ void k_data_fft_rows<R>(const double*, double2*, int, const double2*, R);
PPF_INST_DATA_FFT(RowSmooth<1024>)
PPF_INST_DATA_FFT(RowSmooth<4096>)

// The data pass's per-subint part (k_data_xspec's outputs for any nbin) from
// the spectra k_dft_rows_mfma or k_data_fft_rows left in the X rows -- or, with the data-spectrum
// cache (a.D), in the cache's rows: sig, dsum, the guess average R (each R_k
// summed by one thread in channel order) and X = D conj(M) (0 at k = 0 and
// past nbin/2), in place or into X.  As k_data_xspec: under PPF_SPEC_STORE /
// _USE the Taylor-path subints get no X (their moment passes form it from
// D), under _USE they are not visited at all, and STORE leaves masked rows
// and the padding of the cached D rows zero.
__global__ __launch_bounds__(kBlock) void k_data_post_gen(SpecArgs a, int nbin) {
  __shared__ double s_meta[4];
  __shared__ double red[kWaves];
  const int c = blockIdx.x, s = a.sub0 + c, tid = threadIdx.x;
  const bool tsub = a.D && spec_taylor_sub(a, s);
  if (a.spec_mode == PPF_SPEC_USE && tsub) return;  // all of it cached
  const bool wx = !tsub;                                      // X rows wanted
  const bool wd = a.D != nullptr && a.spec_mode == PPF_SPEC_STORE;  // cache rows to tidy
  const int nchan = a.nchan, NH = nbin / 2 + 1;
  const double* fr = a.freqs + (size_t)s * nchan;
  const uint8_t* mask = a.mask ? a.mask + (size_t)s * nchan : nullptr;
  if (tid == 0) {
    double fs = 0.0, ws = 0.0;
    int nok = 0;
    for (int q = 0; q < nchan; ++q) {
      if (mask && !mask[q]) continue;
      fs += fr[q];
      ws += a.weights ? a.weights[(size_t)s * nchan + q] : 1.0;
      ++nok;
    }
    double nug = a.guess_nu ? a.guess_nu[s] : NAN;
    if (isnan(nug)) nug = fs / nok;
    s_meta[0] = nug;
    s_meta[1] = ws;
    s_meta[2] = (double)nok;
    s_meta[3] = a.init ? a.init[(size_t)s * 5 + 1] : 0.0;
  }
  __syncthreads();
  const double nug2 = 1.0 / (s_meta[0] * s_meta[0]);
  const double wsum = s_meta[1];
  const double Dfac = kDconst * s_meta[3] / a.P[s];
  const int midx = a.model_idx ? a.model_idx[s] : 0;
  double2* Rr = a.R + (size_t)c * a.NHP;
  if (a.guess)
    for (int k = tid; k < a.NHP; k += kBlock) Rr[k] = cmk(0.0, 0.0);
  for (int n = 0; n < nchan; ++n) {
    double2* Xr = a.X + ((size_t)c * nchan + n) * a.NHP;
    double2* Dr = a.D ? a.D + ((size_t)c * nchan + n) * a.NHP : Xr;  // the spectra
    if (mask && !mask[n]) {
      if (tid == 0) { a.sig[(size_t)c * nchan + n] = 0.0; a.dsum[(size_t)c * nchan + n] = 0.0; }
      for (int k = tid; k < a.NHP; k += kBlock) {
        if (wx) Xr[k] = cmk(0.0, 0.0);
        if (wd) Dr[k] = cmk(0.0, 0.0);
      }
      continue;
    }
    const double2* Mr = a.M + ((size_t)midx * nchan + n) * a.NHP;
    const double phi = Dfac * (1.0 / (fr[n] * fr[n]) - nug2);
    const double wq = a.weights ? a.weights[(size_t)s * nchan + n] : 1.0;
    double pn = 0.0, pd = 0.0;
    for (int k = tid; k < a.NHP; k += kBlock) {
      double2 xk = cmk(0.0, 0.0);
      if (k < NH) {
        const double2 d = Dr[k];
        const double p2 = cabs2(d);
        if (k >= a.kc) pn += p2;
        if (k >= 1) pd += p2;
        if (k >= 1) xk = cmulc(d, Mr[k]);
        if (a.guess) Rr[k] = cadd(Rr[k], cmul(d, cscale(turn_phasor((double)k, phi), wq)));
      } else if (wd) {
        Dr[k] = cmk(0.0, 0.0);
      }
      if (wx) Xr[k] = xk;
    }
    pn = block_sum(pn, red);
    pd = block_sum(pd, red);
    if (tid == 0) {
      double sig = a.errs ? a.errs[(size_t)s * nchan + n] : NAN;
      if (isnan(sig)) sig = sqrt(pn / (double)nbin / (double)(NH - a.kc));
      a.sig[(size_t)c * nchan + n] = sig;
      a.dsum[(size_t)c * nchan + n] = pd;
    }
  }
  if (a.guess) {
    const double iw = 1.0 / wsum;
    for (int k = tid; k < a.NHP; k += kBlock) {
      double2 r = cmk(0.0, 0.0);
      if (k < NH) {
        r = cscale(Rr[k], iw);
        if (k == 0) r = cmk(0.0, 0.0);
        if (!(nbin & 1) && k == nbin / 2) r.y = 0.0;
      }
      Rr[k] = r;
    }
  }
}

}  // namespace ppf
