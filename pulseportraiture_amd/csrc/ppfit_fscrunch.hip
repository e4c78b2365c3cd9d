// ppfit_fscrunch.hip -- rotate and frequency-scrunch (gfx950): the weighted
// sum over channels per unit, the transpose of ppalign's rotate-and-sum
// (k_rot_accum sums over subints per channel).
//
// For units u (an archive or a subint), channels n, harmonics k <= nbin/2:
//   P_u[k]  = sum_n w[u][n] rfft(x[u][n])_k e^{2 pi i k phase[u][n]}
//   prof[u] = irfft(P_u, n = nbin)
// i.e. sum_n w[u][n] rotate_rows(x[u][n], phase[u][n]): the dedispersed,
// weighted fscrunch that gives one profile per unit (psradd -P aligns on
// those profiles, make_constant_portrait(profile=None) copies them).  The
// data are read once and nunit * nbin doubles written; rotate_rows and a
// reduction would write and read a rotated copy of the data in between.
//
// One workgroup takes one (unit, channel slice): kFsSlice consecutive
// channels, a constant of the build that never depends on nunit, summed in
// channel order by the thread that owns the harmonic (no atomics).  The
// slices' partial spectra go to the workspace; k_fscrunch_reduce adds them in
// slice order, drops Im P_0 and Im P_{nbin/2} and the irfft follows.  A
// unit's profile is therefore bitwise the same whatever else shares the call.
//
// ppf_scrunch_subints (the stand-in for pam's -f / -b) is the same sum over
// groups of f adjacent channels: fp64 subints [nsub][npol][nchan][nbin] ARE
// units [nsub npol ngroup][f][nbin], so the kernels above run unchanged, and
// 16-bit PSRFITS samples are read by the *_raw twins of the two power-of-two
// kernels -- the same bodies with another row source (FsRaw: RawWaveRow's
// conversion, fma(raw, scl, offs) plus the second polarisation's when two are
// summed, k_unpack's values bit for bit), so raw input gives the bits of
// unpack-then-sum with no fp64 copy of the data.  k_scrunch_meta lays the
// [nsub][nchan] weights and phases out per unit and sums W; k_scrunch_mean
// divides the profile by W and takes the mean of every b adjacent bins.
#include "ppfit_kernels.hpp"

namespace ppf {

// Where a unit's rows come from: fp64 rows [nunit][nchan][nbin] ...
struct FsF64 {
  const double* data;
};
// ... or 16-bit samples (FsRaw, ppfit_kernels.hpp): the stored rows (m0, and
// m1 when two polarisations are summed) of the unit's channel 0; channel n is
// row m + n.
__device__ __forceinline__ void fs_raw_rows(const FsRaw& a, int u, int f, size_t& m0, size_t& m1) {
  const int64_t U = a.unit0 + u;
  const int g = (int)(U % a.ngroup);
  const int64_t r = U / a.ngroup;
  const int q = (int)(r % a.npo);
  const size_t s = (size_t)(r / a.npo);
  const size_t c = (size_t)g * f;
  m0 = (s * a.rnpol + (a.rp0 < 0 ? q : a.rp0)) * a.nchan_all + c;
  m1 = a.rsum ? (s * a.rnpol + a.rp1) * a.nchan_all + c : m0;
}

// partial[(u nslice + p)][k] = sum_{n in slice p} w[u][n] rfft(x[u][n])_k e^{2 pi i k ph[u][n]}
template <int LOGN, class Src>
__device__ __forceinline__ void fscrunch_lds(const Src& src, const double* __restrict__ phase,
                                             const double* __restrict__ weight,
                                             double2* __restrict__ partial, int nchan, int nslice,
                                             const double2* __restrict__ tw) {
  constexpr int N = 1 << LOGN;
  constexpr int KI = (N + 1 + kBlock - 1) / kBlock;
  constexpr bool RAW = std::is_same_v<Src, FsRaw>;
  __shared__ double2 buf[N];
  const int u = blockIdx.x / nslice;
  const int p = blockIdx.x % nslice;
  const int n0 = p * kFsSlice, n1 = min(nchan, n0 + kFsSlice);
  size_t m0 = 0, m1 = 0;
  if constexpr (RAW) fs_raw_rows(src, u, nchan, m0, m1);
  double2 acc[KI];
#pragma unroll
  for (int i = 0; i < KI; ++i) acc[i] = cmk(0.0, 0.0);
  for (int n = n0; n < n1; ++n) {
    const size_t row = (size_t)u * nchan + n;
    const double w = weight[row];
    if (w == 0.0) continue;  // uniform per block
    if constexpr (RAW) {
      const bool sum = src.rsum != 0;
      const typename RawWaveRow<LOGN>::Conv cv(src.scl[m0 + n], src.offs[m0 + n], src.scl[m1 + n],
                                               src.offs[m1 + n], sum);
      const uint32_t* w0 = src.raw + (m0 + n) * N;
      const uint32_t* w1 = src.raw + (m1 + n) * N;
#pragma unroll
      for (int c = 0; c < (N + kBlock - 1) / kBlock; ++c) {
        const int j = threadIdx.x + c * kBlock;
        if (j < N) buf[j] = cv(ld_stream(w0 + j), sum ? ld_stream(w1 + j) : 0u);
      }
    } else {
      load_row<LOGN>(buf, src.data + row * 2 * N);
    }
    __syncthreads();
    lds_fft<LOGN, false>(buf, tw);
    const double ph = phase[row];
#pragma unroll
    for (int i = 0; i < KI; ++i) {
      const int k = threadIdx.x + i * kBlock;
      if (k <= N)
        acc[i] = cadd(acc[i], cscale(cmul(rfft_post<LOGN>(buf, k, tw), turn_phasor((double)k, ph)), w));
    }
    __syncthreads();
  }
  double2* out = partial + (size_t)blockIdx.x * (N + 1);
#pragma unroll
  for (int i = 0; i < KI; ++i) {
    const int k = threadIdx.x + i * kBlock;
    if (k <= N) out[k] = acc[i];
  }
}

template <int LOGN>
__global__ __launch_bounds__(kBlock) void k_fscrunch(const double* __restrict__ data,
                                                     const double* __restrict__ phase,
                                                     const double* __restrict__ weight,
                                                     double2* __restrict__ partial, int nchan,
                                                     int nslice, const double2* __restrict__ tw) {
  fscrunch_lds<LOGN>(FsF64{data}, phase, weight, partial, nchan, nslice, tw);
}
template <int LOGN>
__global__ __launch_bounds__(kBlock) void k_fscrunch_raw(FsRaw src,
                                                         const double* __restrict__ phase,
                                                         const double* __restrict__ weight,
                                                         double2* __restrict__ partial, int nchan,
                                                         int nslice,
                                                         const double2* __restrict__ tw) {
  fscrunch_lds<LOGN>(src, phase, weight, partial, nchan, nslice, tw);
}

// The same sum for nbin = 2048 with the register FFT, as k_rot_accum_w has it
// (ppfit_spectra.hip): the workgroup's four waves take channels n0 + w, n0 +
// w + 4, ... of the slice, one row per wave per group of four (fft1024_wave
// into the wave's own LDS buffer, the next row's load started after stage
// A); after a barrier every wave adds the group's four rows, in channel
// order, into the harmonic pairs it owns (k = lane + 64 j and N - k for j =
// w, w + 4, w + 8, j <= 8).  The rotation w e^{2 pi i k ph}: turn_phasor at
// k = lane + 64 w per row, stepped by e^{2 pi i 256 ph}; the row's own wave
// forms that step and e^{2 pi i N ph} once and passes them through LDS.
template <class Src>
__device__ __forceinline__ void fscrunch_wave(const Src& src, const double* __restrict__ phase,
                                              const double* __restrict__ weight,
                                              double2* __restrict__ partial, int nchan, int nslice,
                                              const double2* __restrict__ tw) {
  constexpr int LOGN = 10, N = 1 << LOGN, NJ = 3;  // j = w + 4 i <= 8
  constexpr bool RAW = std::is_same_v<Src, FsRaw>;
  static_assert(kFsSlice <= 4 * 64, "one lane per group of four channels");
  __shared__ double2 bufs[4][kFft1024Slots];
  __shared__ Fft1024Tw ftw;
  __shared__ double2 s_step[4], s_EN[4];
  __shared__ double s_w[4], s_ph[4];
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int u = blockIdx.x / nslice, p = blockIdx.x % nslice;
  const int n0 = p * kFsSlice, n1 = min(nchan, n0 + kFsSlice);
  const int ngrp = (n1 - n0 + 3) / 4;
  const size_t base = (size_t)u * nchan;
  ftw.fill(tw, tid, 256);
  double2* buf = bufs[w];
  double2 ak[NJ], an[NJ], tk[NJ];
#pragma unroll
  for (int i = 0; i < NJ; ++i) {
    ak[i] = an[i] = cmk(0.0, 0.0);
    double sw, cw;  // rfft post-processing twiddle e^{-i pi k / N} of pair k
    sincospi(-(double)(lane + 64 * (w + 4 * i)) / (double)N, &sw, &cw);
    tk[i] = cmk(cw, sw);
  }
  size_t m0 = 0, m1 = 0;
  if constexpr (RAW) fs_raw_rows(src, u, nchan, m0, m1);
  auto rowp = [&](int n) {
    if constexpr (RAW) {
      return RawRowSrc{src.raw + (m0 + n) * N, src.raw + (m1 + n) * N,
                       ((lane & 1) ? src.offs : src.scl) + ((lane & 2) ? m1 : m0) + n};
    } else {
      return src.data + (base + n) * 2 * N;
    }
  };
  // weight and phase of this wave's row of every group (lane l: group l), as
  // vector loads: a scalar load per row would hold up the FFT's LDS waits
  double wv, pv;
  {
    const int n = n0 + 4 * lane + w;
    const size_t i = base + (n < n1 ? n : n0);
    wv = n < n1 ? weight[i] : 0.0;
    pv = phase[i];
  }
  std::conditional_t<RAW, RawWaveRow<LOGN>, WaveRow<LOGN>> row;
  if constexpr (RAW) row.sum = src.rsum != 0;
  if (n0 + w < n1) row.load(rowp(n0 + w), lane);
  __syncthreads();  // ftw
  for (int t = 0; t < ngrp; ++t) {
    const int nn = n0 + 4 * t + w + 4;  // this wave's next row
    const double wc = lane_of(wv, t), pc = lane_of(pv, t);  // 0 past n1
    auto load_next = [&] {
      if (nn < n1) row.load(rowp(nn), lane);
    };
    if (wc != 0.0) {
      if constexpr (RAW) {
        // the packed row is consumed here: its registers are the next row's
        // from load_next on
        double x[16], y[16];
        row.unpack(x, y);
        if constexpr (PPF_EARLY_ROW) {
          fft1024_wave(x, y, buf, ftw, lane, load_next);
        } else {
          fft1024_wave(x, y, buf, ftw, lane);
          load_next();
        }
      } else if constexpr (PPF_EARLY_ROW) {
        fft1024_wave(row.x, row.y, buf, ftw, lane, load_next);
      } else {
        fft1024_wave(row.x, row.y, buf, ftw, lane);
        load_next();
      }
      const double2 st = turn_phasor(256.0, pc), en = turn_phasor((double)N, pc);
      if (lane == 0) { s_step[w] = st; s_EN[w] = en; s_ph[w] = pc; }
    } else {
      load_next();
    }
    if (lane == 0) s_w[w] = wc;
    __syncthreads();  // the group's four spectra and their rotations
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const double wr = s_w[r];
      if (wr != 0.0) {  // uniform per workgroup
        const double pr = s_ph[r];
        const double2 st = s_step[r], EN = s_EN[r];
        const double2* br = bufs[r];
        double2 e = cscale(turn_phasor((double)(lane + 64 * w), pr), wr);
#pragma unroll
        for (int i = 0; i < NJ; ++i) {
          const int k = lane + 64 * (w + 4 * i);
          if (i > 0) e = cmul(e, st);
          if (k <= N / 2) {
            double2 xk, xn;
            rfft_pair_v(br[fft1024_slot(k)], br[fft1024_slot((N - k) & (N - 1))], tk[i], xk, xn);
            ak[i] = cadd(ak[i], cmul(xk, e));
            if (k < N / 2) an[i] = cadd(an[i], cmul(xn, cmul(EN, cconj(e))));
          }
        }
      }
    }
    __syncthreads();  // buffers and the row table free for the next group
  }
  double2* out = partial + (size_t)blockIdx.x * (N + 1);
#pragma unroll
  for (int i = 0; i < NJ; ++i) {
    const int k = lane + 64 * (w + 4 * i);
    if (k <= N / 2) {
      out[k] = ak[i];
      if (k < N / 2) out[N - k] = an[i];  // k = 0: the Nyquist harmonic
    }
  }
}

__global__ __launch_bounds__(256, 2) void k_fscrunch_w(const double* __restrict__ data,
                                                      const double* __restrict__ phase,
                                                      const double* __restrict__ weight,
                                                      double2* __restrict__ partial, int nchan,
                                                      int nslice,
                                                      const double2* __restrict__ tw) {
  fscrunch_wave(FsF64{data}, phase, weight, partial, nchan, nslice, tw);
}
__global__ __launch_bounds__(256, 2) void k_fscrunch_w_raw(FsRaw src,
                                                          const double* __restrict__ phase,
                                                          const double* __restrict__ weight,
                                                          double2* __restrict__ partial,
                                                          int nchan, int nslice,
                                                          const double2* __restrict__ tw) {
  fscrunch_wave(src, phase, weight, partial, nchan, nslice, tw);
}

// The same for any nbin (RowAny's direct sums): thread t sums harmonics
// k = t, t + kBlock, ... in channel order, in its own cells of the partial
// spectrum (k_rot_accum<RowAny>'s loop, over channels).  Dynamic LDS:
// RowAny::lds(nbin, kLdsRow).
__global__ __launch_bounds__(kBlock) void k_fscrunch_gen(const double* __restrict__ data,
                                                         const double* __restrict__ phase,
                                                         const double* __restrict__ weight,
                                                         double2* __restrict__ partial, int nchan,
                                                         int nslice,
                                                         const double2* __restrict__ tw,
                                                         RowAny rw) {
  __shared__ RowAny::Lds<kLdsRow> sm;
  RowAny::Dev t(rw, sm, tw);
  const int u = blockIdx.x / nslice, p = blockIdx.x % nslice;
  const int n0 = p * kFsSlice, n1 = min(nchan, n0 + kFsSlice);
  RowAny::Own acc(partial + (size_t)blockIdx.x * t.nh());
  t.for_bins([&](int i, int k) { acc.at(i, k) = cmk(0.0, 0.0); });
  for (int n = n0; n < n1; ++n) {
    const size_t row = (size_t)u * nchan + n;
    const double w = weight[row];
    if (w == 0.0) continue;  // uniform per block
    t.load(data + row * t.nbin());
    rot_add(t, acc, phase[row], w);
    t.release();
  }
}

// spec[u][k] = sum_p partial[u nslice + p][k] in slice order, k <= nbin/2 (NH
// cells per row); irfft keeps only the real part of the DC and, for an even
// nbin (nyq = nbin/2, else -1), the Nyquist term.
__global__ void k_fscrunch_reduce(const double2* __restrict__ partial, double2* __restrict__ spec,
                                  int nslice, int NH, int nyq, size_t count) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const size_t u = i / NH;
  const int k = (int)(i - u * NH);
  const double2* pu = partial + u * nslice * NH + k;
  double2 s = cmk(0.0, 0.0);
  for (int p = 0; p < nslice; ++p) s = cadd(s, pu[(size_t)p * NH]);
  if (k == 0 || k == nyq) s.y = 0.0;
  spec[i] = s;
}

// ppf_scrunch_subints: the [nsub][nchan_all] weights and phases laid out per
// unit (unit0 + i = (s npo + q) ngroup + g takes channels g f .. g f + f - 1
// of subint s), the unit's W = sum_n w summed in channel order, and wout[s][g]
// = W (written by the unit of q = 0).  One thread per unit.
__global__ void k_scrunch_meta(const double* __restrict__ weights,
                               const double* __restrict__ phase, int64_t unit0, int nu, int npo,
                               int ngroup, int f, double* __restrict__ wx,
                               double* __restrict__ phx, double* __restrict__ Wx,
                               double* __restrict__ wout) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nu) return;
  const int64_t U = unit0 + i;
  const int g = (int)(U % ngroup);
  const int64_t r = U / ngroup;
  const size_t s = (size_t)(r / npo);
  const size_t src = (s * ngroup + g) * f;
  double W = 0.0;
  for (int n = 0; n < f; ++n) {
    const double w = weights[src + n];
    wx[(size_t)i * f + n] = w;
    phx[(size_t)i * f + n] = phase[src + n];
    W += w;
  }
  Wx[i] = W;
  if (r % npo == 0) wout[s * ngroup + g] = W;
}

// out[u][j] = (1/b) sum_{i < b} prof[u][j b + i] / W[u]; zeros where W = 0.
__global__ void k_scrunch_mean(const double* __restrict__ prof, const double* __restrict__ Wx,
                               double* __restrict__ out, int nbin, int b, size_t count) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const int nbo = nbin / b;
  const size_t u = i / nbo;
  const int j = (int)(i - u * nbo);
  const double W = Wx[u];
  double s = 0.0;
  if (W != 0.0) {
    const double* y = prof + u * nbin + (size_t)j * b;
    for (int t = 0; t < b; ++t) s += y[t] / W;
    s = s / (double)b;
  }
  out[i] = s;
}

#define PPF_INST_FS(L)                                                                     \
  template __global__ void k_fscrunch<L>(const double*, const double*, const double*,      \
                                         double2*, int, int, const double2*);              \
  template __global__ void k_fscrunch_raw<L>(FsRaw, const double*, const double*, double2*, \
                                             int, int, const double2*);
PPF_INST_FS(5)
PPF_INST_FS(6)
PPF_INST_FS(7)
PPF_INST_FS(8)
PPF_INST_FS(9)
PPF_INST_FS(10)
PPF_INST_FS(11)
PPF_INST_FS(12)

}  // namespace ppf
