// ppfit_rowfft.hpp -- the row transform of the rfft-based row kernels as a
// policy: RowPow2<LOGN> (nbin = 2^(LOGN + 1) from 64 up: the LDS FFT of
// ppfit_device.hpp), RowSmooth<MAXN> (even nbin with nbin / 2 = 2^a 3^b 5^c <=
// MAXN: the mixed-radix LDS FFT of ppfit_smoothfft.hpp) and RowAny (every
// other nbin in [16, 8192]: direct sums, O(nbin^2) per row).  A row kernel is
// one `template <class Row>` body; what differs between them -- how a bin is
// obtained, how a spectrum goes back to samples, where a thread keeps the
// bins it owns, the LDS -- is here.
//
// Bin k of a real row: D_k = sum_m x_m e^{-2 pi i m k / nbin}.  The direct
// sums take one bin per thread, the phasor advancing by one complex product
// per term and re-seeded from the twiddle table at the exact index (m k) mod
// nbin every kSeed terms, so its rounding never grows past kSeed products
// (relative error ~1e-15, against the north_star tolerance of 1e-3 sigma on
// the fitted parameters).
#pragma once
#include "ppfit_device.hpp"
#include "ppfit_smoothfft.hpp"

namespace ppf {

// ---------------------------------------------------------------------------
// power of two: packed complex row, LDS FFT, rfft_post / irfft_pre
// ---------------------------------------------------------------------------
// Load a real row of 2N doubles as N packed complex values into LDS.
template <int LOGN>
__device__ __forceinline__ void load_row(double2* buf, const double* __restrict__ row) {
  constexpr int N = 1 << LOGN;
  const double2* r2 = reinterpret_cast<const double2*>(row);
#pragma unroll
  for (int c = 0; c < (N + kBlock - 1) / kBlock; ++c) {
    const int j = threadIdx.x + c * kBlock;
    if (j < N) buf[j] = r2[j];
  }
}

// epi(j, v): the value stored at complex sample j (bins 2j, 2j + 1), given
// the transform's v -- a fused epilogue (k_synth adds its noise there).
// active(): false when epi is the identity for this row (RowAny then skips
// its second pass over the samples).
struct C2rPlain {
  template <class V>
  __device__ double2 operator()(int, V v) const { return v; }
  __device__ constexpr bool active() const { return false; }
};
// The transform alone: buf[j] (j in [0, N)) is left holding N times the sample
// pair (2j, 2j + 1); the caller synchronises nothing more before reading its
// own j = tid + i kBlock.
template <int LOGN>
__device__ void c2r_in_lds(double2* buf, double2 (&xs)[((1 << LOGN) + kBlock) / kBlock + 1],
                           const double2* __restrict__ tw) {
  constexpr int N = 1 << LOGN;
  constexpr int KI = (N + 1 + kBlock - 1) / kBlock;
  const int tid = threadIdx.x;
  // stage X_k (k in [0, N]) in LDS, then form Z_k for k in [0, N)
#pragma unroll
  for (int i = 0; i < KI; ++i) {
    const int k = tid + i * kBlock;
    if (k <= N) {
      double2 x = xs[i];
      if (k == 0 || k == N) x.y = 0.0;
      buf[k] = x;
    }
  }
  __syncthreads();
  double2 z[KI];
#pragma unroll
  for (int i = 0; i < KI; ++i) {
    const int k = tid + i * kBlock;
    if (k < N) z[i] = irfft_pre<LOGN>(buf[k], buf[N - k], k, tw);
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < KI; ++i) {
    const int k = tid + i * kBlock;
    if (k < N) buf[k] = z[i];
  }
  __syncthreads();
  lds_fft<LOGN, true>(buf, tw);
}

template <int LOGN, typename Epi = C2rPlain>
__device__ void c2r_from_spectrum(double2* buf, double2 (&xs)[((1 << LOGN) + kBlock) / kBlock + 1],
                                  const double2* __restrict__ tw, double* __restrict__ out,
                                  Epi epi = Epi()) {
  constexpr int N = 1 << LOGN;
  c2r_in_lds<LOGN>(buf, xs, tw);
  const double inv = 1.0 / (double)N;
  double2* o2 = reinterpret_cast<double2*>(out);
  for (int j = threadIdx.x; j < N; j += kBlock) o2[j] = epi(j, cscale(buf[j], inv));
}

// ---------------------------------------------------------------------------
// any nbin: direct sums
// ---------------------------------------------------------------------------
constexpr int kSeed = 32;

// D_k of x[0 .. nbin) (LDS); tw[j] = e^{-2 pi i j / nbin}, k < nbin.  The
// real input's symmetry halves the work: terms m and nbin - m share the
// phasor, D_k = x_0 + sum_{1 <= m < nbin/2} [(x_m + x_{nbin-m}) cos -
// i (x_m - x_{nbin-m}) sin](2 pi m k / nbin) + [nbin even] (-1)^k x_{nbin/2}.
__device__ __forceinline__ double2 dft_bin(const double* x, int nbin, int k,
                                           const double2* __restrict__ tw) {
  const double2 w = tw[k];
  const int M = (nbin - 1) / 2;  // pairs m = 1 .. M
  const int step = (int)(((long long)kSeed * k) % nbin);
  double re = x[0], im = 0.0;
  int seed = k;  // (m0 k) mod nbin at m0 = 1
  for (int m0 = 1; m0 <= M; m0 += kSeed) {
    double2 e = tw[seed];
    const int me = min(m0 + kSeed - 1, M);
    for (int m = m0; m <= me; ++m) {
      const double a = x[m], b = x[nbin - m];
      re = fma(a + b, e.x, re);
      im = fma(a - b, e.y, im);
      e = cmul(e, w);
    }
    seed += step;
    if (seed >= nbin) seed -= nbin;
  }
  if (!(nbin & 1)) re += (k & 1) ? -x[nbin / 2] : x[nbin / 2];
  return cmk(re, im);
}

// numpy irfft(X, n = nbin) at samples m and nbin - m (1 <= m < nbin/2):
// with A = sum_{1 <= k <= K} Re X_k cos(2 pi m k / nbin) and B = sum Im X_k
// sin(..), K = (nbin - 1) / 2, the two samples are (Re X_0 + 2 (A -+ B) +
// [nbin even] (-1)^m Re X_{nbin/2}) / nbin; m = 0 (and m = nbin/2) alone,
// with B = 0.  X[0 .. nbin/2] in LDS.
__device__ __forceinline__ void idft_pair(const double2* X, int nbin, int m,
                                          const double2* __restrict__ tw, double& out_m,
                                          double& out_nm) {
  const double2 w = cconj(tw[m]);  // e^{+2 pi i m / nbin}
  const int K = (nbin - 1) / 2;
  const int step = (int)(((long long)kSeed * m) % nbin);
  double A = 0.0, B = 0.0;
  int seed = m;  // (k0 m) mod nbin at k0 = 1
  for (int k0 = 1; k0 <= K; k0 += kSeed) {
    double2 e = cconj(tw[seed]);
    const int ke = min(k0 + kSeed - 1, K);
    for (int k = k0; k <= ke; ++k) {
      const double2 x = X[k];
      A = fma(x.x, e.x, A);
      B = fma(x.y, e.y, B);
      e = cmul(e, w);
    }
    seed += step;
    if (seed >= nbin) seed -= nbin;
  }
  double ny = 0.0;
  if (!(nbin & 1)) ny = (m & 1) ? -X[nbin / 2].x : X[nbin / 2].x;
  const double inv = 1.0 / (double)nbin;
  out_m = (fma(2.0, A - B, X[0].x) + ny) * inv;
  out_nm = (fma(2.0, A + B, X[0].x) + ny) * inv;
}

// every sample of irfft(X, n = nbin) into out[0 .. nbin), the block's threads
// taking the pairs (m, nbin - m)
__device__ __forceinline__ void idft_row(const double2* X, int nbin, const double2* __restrict__ tw,
                                         double* __restrict__ out) {
  const int half = nbin / 2;
  for (int m = threadIdx.x; m <= half; m += blockDim.x) {
    double a, b;
    idft_pair(X, nbin, m, tw, a, b);
    out[m] = a;
    if (m > 0 && nbin - m != m) out[nbin - m] = b;
  }
}

__device__ __forceinline__ void load_real_row(double* x, const double* __restrict__ row, int nbin) {
  for (int m = threadIdx.x; m < nbin; m += blockDim.x) x[m] = row[m];
}

// v / (1 + i w): the scattering kernel's divide at w = 2 pi k tau
// (scattering_portrait_FT, pplib.py:4081-4101)
__device__ __forceinline__ double2 scat_div(double2 v, double w) {
  const double d = 1.0 / fma(w, w, 1.0);
  return cmk(fma(v.y, w, v.x) * d, fma(-v.x, w, v.y) * d);
}

// ---------------------------------------------------------------------------
// The policy.  A kernel holds, as its argument, a Row (nothing, or nbin) and
// builds the device view from it:
//   __shared__ typename Row::template Lds<U> sm;   // U: what the kernel keeps
//   typename Row::Dev t(row, sm, tw);
//   t.load(p)        the row at p, transformed; then bin(k), k < nh()
//   t.release()      every thread has taken its bins: load() may follow
//   t.for_bins(f)    f(i, k) for the bins the thread owns, k = tid + i kBlock
//   Row::Own         the thread's owned bins between two passes: registers
//                    (RowPow2, RowSmooth) or the cells of a spectrum in memory
//                    (RowAny)
//   t.inverse(own, out, epi)   out = epi(irfft of the owned bins)
// The launch passes Row::lds(nbin, U) bytes of dynamic LDS.
// ---------------------------------------------------------------------------
enum RowLds {
  kLdsRow,      // a row to transform
  kLdsSpec,     // one spectrum to transform back (or a row and, in its place, nh() pairs)
  kLdsRowInv,   // a row, transformed, changed and transformed back
  kLdsRowSpec,  // a row and beside it a spectrum that every thread reads
};

template <int LOGN>
struct RowPow2 {
  static constexpr int kLogN = LOGN, N = 1 << LOGN, NH = N + 1;
  static constexpr int KI = (NH + kBlock - 1) / kBlock;  // bins per thread
  static constexpr int kMaxKI = KI;
  static constexpr bool kFft = true;  // the inverse runs in the row's own buffer
  template <RowLds U>
  struct Lds {
    double2 buf[U == kLdsRow ? N : N + 1];
    double2 spec[U == kLdsRowSpec ? N + 1 : 0];
  };
  static size_t lds(int, RowLds) { return 0; }  // static arrays

  struct Own {
    double2 v[(N + kBlock) / kBlock + 1];
    __device__ __forceinline__ Own(double2*) {}
    __device__ __forceinline__ double2& at(int i, int) { return v[i]; }
  };

  struct Dev {
    double2 *buf, *spec;
    const double2* tw;
    template <RowLds U>
    __device__ __forceinline__ Dev(RowPow2, Lds<U>& sm, const double2* tw_)
        : buf(sm.buf), spec(sm.spec), tw(tw_) {}
    __device__ __forceinline__ constexpr int nbin() const { return 2 * N; }
    __device__ __forceinline__ constexpr int nh() const { return NH; }
    __device__ __forceinline__ void load(const double* __restrict__ row) {
      load_row<LOGN>(buf, row);
      __syncthreads();
      lds_fft<LOGN, false>(buf, tw);
    }
    __device__ __forceinline__ double2 bin(int k) const { return rfft_post<LOGN>(buf, k, tw); }
    __device__ __forceinline__ void release() { __syncthreads(); }
    __device__ __forceinline__ double* reals() { return reinterpret_cast<double*>(buf); }
    template <class F>
    __device__ __forceinline__ void for_bins(F&& f) {
#pragma unroll
      for (int i = 0; i < KI; ++i) {
        const int k = threadIdx.x + i * kBlock;
        if (k <= N) f(i, k);
      }
    }
    template <class Epi = C2rPlain>
    __device__ __forceinline__ void inverse(Own& own, double* __restrict__ out, Epi epi = Epi()) {
      c2r_from_spectrum<LOGN>(buf, own.v, tw, out, epi);
    }
  };
};

// a sample pair already in memory, read when the epilogue asks for it
struct StoredPair {
  const double* p;
  bool two;
  __device__ __forceinline__ operator double2() const { return cmk(p[0], two ? p[1] : 0.0); }
};

struct RowAny {
  int n;
  static constexpr int kMaxKI = (8192 / 2 + 1 + kBlock - 1) / kBlock;
  static constexpr bool kFft = false;
  template <RowLds U>
  struct Lds {};  // dynamic
  __host__ __device__ static size_t row_bytes(int nbin) {
    return ((size_t)nbin * sizeof(double) + 15) & ~(size_t)15;
  }
  static size_t lds(int nbin, RowLds u) {
    const size_t spec = (size_t)(nbin / 2 + 1) * sizeof(double2);
    if (u == kLdsRow) return (size_t)nbin * sizeof(double);
    return u == kLdsSpec ? spec : row_bytes(nbin) + spec;
  }

  struct Own {
    double2* X;
    __device__ __forceinline__ Own(double2* cells) : X(cells) {}
    __device__ __forceinline__ double2& at(int, int k) { return X[k]; }
  };

  struct Dev {
    double* x;      // the row
    double2* spec;  // the spectrum (kLdsSpec: in the row's place)
    const double2* tw;
    int n;
    template <RowLds U>
    __device__ __forceinline__ Dev(RowAny row, Lds<U>&, const double2* tw_) : tw(tw_), n(row.n) {
      extern __shared__ __align__(16) unsigned char gsm[];
      x = reinterpret_cast<double*>(gsm);
      spec = reinterpret_cast<double2*>(gsm + (U == kLdsSpec ? 0 : row_bytes(n)));
    }
    __device__ __forceinline__ int nbin() const { return n; }
    __device__ __forceinline__ int nh() const { return n / 2 + 1; }
    __device__ __forceinline__ void load(const double* __restrict__ row) {
      load_real_row(x, row, n);
      __syncthreads();
    }
    __device__ __forceinline__ double2 bin(int k) const { return dft_bin(x, n, k, tw); }
    __device__ __forceinline__ void release() { __syncthreads(); }
    __device__ __forceinline__ double* reals() { return x; }
    template <class F>
    __device__ __forceinline__ void for_bins(F&& f) {
      const int NH = nh();
      for (int k = threadIdx.x, i = 0; k < NH; k += kBlock, ++i) f(i, k);
    }
    // the owned bins are cells of `spec`.  Sample pairs (2j, 2j + 1) and the
    // pairs (m, nbin - m) of idft_row belong to different threads, so the
    // epilogue is a second pass over the stored row.
    template <class Epi = C2rPlain>
    __device__ __forceinline__ void inverse(Own&, double* __restrict__ out, Epi epi = Epi()) {
      __syncthreads();
      idft_row(spec, n, tw, out);
      if (!epi.active()) return;
      __syncthreads();  // the block's samples are stored (each pair is then one thread's)
      for (int j = threadIdx.x; 2 * j < n; j += kBlock) {
        const bool two = 2 * j + 1 < n;  // odd nbin: the last sample takes its pair's first normal
        const double2 v = epi(j, StoredPair{out + 2 * j, two});
        out[2 * j] = v.x;
        if (two) out[2 * j + 1] = v.y;
      }
    }
  };
};

// ---------------------------------------------------------------------------
// nbin / 2 = 2^a 3^b 5^c: the mixed-radix LDS FFT
// ---------------------------------------------------------------------------
// One pass of the Stockham FFT of N points in buf, all kBlock threads: every
// butterfly's inputs to registers, a barrier, the outputs to their places, a
// barrier (lds_fft's passes, the radix and N known at run time; MAXN bounds
// the register arrays).
template <int R, int MAXN, bool INV>
__device__ __forceinline__ void smooth_pass(double2* buf, const double2* __restrict__ tw, int N,
                                            int Ns) {
  constexpr int B = smooth_chunks(MAXN, R);
  const SmoothPass ps(N, R, Ns);
  double2 v[B][R];
#pragma unroll
  for (int c = 0; c < B; ++c) {
    const int j = threadIdx.x + c * kBlock;
    if (j < ps.Q) smooth_gather<R, INV>(buf, tw, ps, j, v[c]);
  }
  __syncthreads();
#pragma unroll
  for (int c = 0; c < B; ++c) {
    const int j = threadIdx.x + c * kBlock;
    if (j < ps.Q) smooth_scatter<R, INV>(buf, ps, j, v[c]);
  }
  __syncthreads();
}

// The transform of plan p in buf (unnormalised both ways, as lds_fft).
template <int MAXN, bool INV>
__device__ void smooth_fft(double2* buf, const double2* __restrict__ tw, const SmoothPlan& p) {
  int Ns = 1;
  for (int s = 0; s < p.npass; ++s) {
    const int r = p.radix(s);  // uniform
    if (r == 4) smooth_pass<4, MAXN, INV>(buf, tw, p.n, Ns);
    else if (r == 2) smooth_pass<2, MAXN, INV>(buf, tw, p.n, Ns);
    else if (r == 3) smooth_pass<3, MAXN, INV>(buf, tw, p.n, Ns);
    else smooth_pass<5, MAXN, INV>(buf, tw, p.n, Ns);
    Ns *= r;
  }
}

// MAXN: the size class (smooth_class), N = nbin / 2 <= MAXN.  The owned bins
// are registers and the inverse runs in the row's own buffer with the
// epilogue per complex sample pair, as RowPow2's.  Dynamic LDS: N + 1 cells
// (N for a row that is only transformed), twice that with a spectrum beside.
template <int MAXN>
struct RowSmooth {
  SmoothPlan plan;
  static constexpr int KI = (MAXN + 1 + kBlock - 1) / kBlock;  // bins per thread
  static constexpr int kMaxKI = KI;
  static constexpr bool kFft = true;
  template <RowLds U>
  struct Lds {};  // dynamic
  static size_t lds(int nbin, RowLds u) {
    const size_t N = (size_t)nbin / 2;
    if (u == kLdsRow) return N * sizeof(double2);
    return (u == kLdsRowSpec ? 2 : 1) * (N + 1) * sizeof(double2);
  }

  struct Own {
    double2 v[KI];
    __device__ __forceinline__ Own(double2*) {}
    __device__ __forceinline__ double2& at(int i, int) { return v[i]; }
  };

  struct Dev {
    double2 *buf, *spec;
    const double2* tw;
    SmoothPlan plan;
    template <RowLds U>
    __device__ __forceinline__ Dev(RowSmooth row, Lds<U>&, const double2* tw_)
        : tw(tw_), plan(row.plan) {
      extern __shared__ __align__(16) unsigned char gsm[];
      buf = reinterpret_cast<double2*>(gsm);
      spec = buf + (U == kLdsRowSpec ? plan.n + 1 : 0);
    }
    __device__ __forceinline__ int nbin() const { return 2 * plan.n; }
    __device__ __forceinline__ int nh() const { return plan.n + 1; }
    __device__ __forceinline__ void load(const double* __restrict__ row) {
      const double2* r2 = reinterpret_cast<const double2*>(row);
      for (int j = threadIdx.x; j < plan.n; j += kBlock) buf[j] = r2[j];
      __syncthreads();
      smooth_fft<MAXN, false>(buf, tw, plan);
    }
    __device__ __forceinline__ double2 bin(int k) const {
      return smooth_rfft_post(buf, plan.n, k, tw[k]);
    }
    __device__ __forceinline__ void release() { __syncthreads(); }
    __device__ __forceinline__ double* reals() { return reinterpret_cast<double*>(buf); }
    template <class F>
    __device__ __forceinline__ void for_bins(F&& f) {
      const int N = plan.n;
#pragma unroll
      for (int i = 0; i < KI; ++i) {
        const int k = threadIdx.x + i * kBlock;
        if (k <= N) f(i, k);
      }
    }
    // c2r_from_spectrum at a run-time N: X_k staged in buf[0 .. N], Z_k formed
    // in registers, the inverse passes, then epi per sample pair
    template <class Epi = C2rPlain>
    __device__ __forceinline__ void inverse(Own& own, double* __restrict__ out, Epi epi = Epi()) {
      const int N = plan.n, tid = threadIdx.x;
#pragma unroll
      for (int i = 0; i < KI; ++i) {
        const int k = tid + i * kBlock;
        if (k <= N) {
          double2 x = own.v[i];
          if (k == 0 || k == N) x.y = 0.0;
          buf[k] = x;
        }
      }
      __syncthreads();
      double2 z[KI];
#pragma unroll
      for (int i = 0; i < KI; ++i) {
        const int k = tid + i * kBlock;
        if (k < N) z[i] = smooth_irfft_pre(buf[k], buf[N - k], tw[k]);
      }
      __syncthreads();
#pragma unroll
      for (int i = 0; i < KI; ++i) {
        const int k = tid + i * kBlock;
        if (k < N) buf[k] = z[i];
      }
      __syncthreads();
      smooth_fft<MAXN, true>(buf, tw, plan);
      const double inv = 1.0 / (double)N;
      double2* o2 = reinterpret_cast<double2*>(out);
      for (int j = tid; j < N; j += kBlock) o2[j] = epi(j, cscale(buf[j], inv));
    }
  };
};

}  // namespace ppf
