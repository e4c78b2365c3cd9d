// ppfit_smoothfft.hpp -- the plan and the passes of the mixed-radix row FFT
// (RowSmooth, ppfit_rowfft.hpp): which nbin take which row transform, the
// list of radices of a length, and one butterfly's gather and scatter with
// their index arithmetic.  Everything here is a plain function of integers
// and of a complex type with members x and y, host and device alike:
// tools/rowfft_plan_check.cpp includes this header in a host program and runs
// the same plan and passes for every eligible length, the threads as a loop.
//
// A real row of nbin = 2 N samples is packed as N complex points z_j =
// (x_2j, x_2j+1).  N = 2^a 3^b 5^c is transformed by a Stockham autosort FFT:
// pass s has radix R_s and span Ns = R_0 ... R_{s-1}; butterfly j < N / R
// reads z[j + q N / R] (q < R), multiplies by e^{-2 pi i q k / (R Ns)} with
// k = j mod Ns, and writes its outputs to (j - k) R + k + q Ns.  The twiddle
// is the exact entry 2 q k (N / (R Ns)) < nbin of the table tw[m] = e^{-2 pi
// i m / nbin} every row kernel already has (k_twiddles): no phasor chains.
// Pass order: one radix-2 pass when a is odd, then the radix-4, radix-3 and
// radix-5 passes.
#pragma once

#include <math.h>

#ifndef PPF_HD
#if defined(__HIPCC__)
#define PPF_HD __host__ __device__
#else
#define PPF_HD
#endif
#endif
#if defined(__HIPCC__)
#define PPF_UNROLL _Pragma("unroll")
#else
#define PPF_UNROLL
#endif

namespace ppf {

// the row transform of a length (include/ppfit.h: PPF_ROW_*)
enum RowKind { kRowPow2 = 0, kRowSmooth = 1, kRowDirect = 2 };

// at most 12 passes: 3^12 > 4096 >= N, and every other radix is larger
constexpr int kSmoothMaxPass = 12;

// The pass plan of a length: N complex points and the radices, four bits
// each, pass s in bits [4 s, 4 s + 4) (a list held in one register pair, so
// a kernel indexes it without an array).
struct SmoothPlan {
  int n;                      // N = nbin / 2
  int npass;
  unsigned long long radices;
  PPF_HD int radix(int s) const { return (int)((radices >> (4 * s)) & 15u); }
};

// The plan of nbin; false when nbin is odd or nbin / 2 has a prime factor
// above 5.
PPF_HD inline bool smooth_plan(int nbin, SmoothPlan* p) {
  if (nbin < 2 || (nbin & 1)) return false;
  int m = nbin / 2, a = 0, b = 0, c = 0;
  while (m % 2 == 0) { m /= 2; ++a; }
  while (m % 3 == 0) { m /= 3; ++b; }
  while (m % 5 == 0) { m /= 5; ++c; }
  if (m != 1) return false;
  p->n = nbin / 2;
  p->npass = 0;
  p->radices = 0;
  auto push = [&](int r, int count) {
    for (int i = 0; i < count; ++i) p->radices |= (unsigned long long)r << (4 * p->npass++);
  };
  push(2, a & 1);
  push(4, a / 2);
  push(3, b);
  push(5, c);
  return true;
}

// The one predicate of the row dispatch: nbin in [16, 8192] (the caller
// checks the range) goes to the power-of-two FFT from 64 up, to the
// mixed-radix FFT when nbin is even with nbin / 2 = 2^a 3^b 5^c and the
// option row_fft is set, and to the direct sums otherwise.
PPF_HD inline RowKind row_kind(int nbin, bool row_fft) {
  if (nbin >= 64 && !(nbin & (nbin - 1))) return kRowPow2;
  SmoothPlan p;
  return row_fft && smooth_plan(nbin, &p) ? kRowSmooth : kRowDirect;
}

// Size classes: a kernel instantiation serves N <= its class, and a thread
// stages at most smooth_chunks(class, R) butterflies of a radix-R pass in
// registers (kBlock = 256 threads: ceil(class / (256 R))).
PPF_HD constexpr int smooth_class(int N) { return N <= 1024 ? 1024 : 4096; }
PPF_HD constexpr int smooth_chunks(int maxn, int R) { return (maxn / R + 255) / 256; }

// j / Ns for j, Ns <= 4096 by one multiply: magic = ceil(2^32 / Ns) errs by
// less than j Ns / 2^32 < 1 / Ns in the quotient.  Ns = 1 has no 32-bit magic.
PPF_HD inline unsigned smooth_magic(int Ns) { return Ns == 1 ? 0u : 0xFFFFFFFFu / (unsigned)Ns + 1u; }
PPF_HD inline int smooth_div(int j, int Ns, unsigned magic) {
  return Ns == 1 ? j : (int)(((unsigned long long)(unsigned)j * magic) >> 32);
}

// complex helpers on any type with x and y (double2 on the device)
template <class C> PPF_HD inline C sm_mk(double x, double y) { C c; c.x = x; c.y = y; return c; }
template <class C> PPF_HD inline C sm_add(C a, C b) { return sm_mk<C>(a.x + b.x, a.y + b.y); }
template <class C> PPF_HD inline C sm_sub(C a, C b) { return sm_mk<C>(a.x - b.x, a.y - b.y); }
template <class C> PPF_HD inline C sm_mul(C a, C b) {
  return sm_mk<C>(fma(a.x, b.x, -a.y * b.y), fma(a.x, b.y, a.y * b.x));
}
// -i a (forward) or +i a (INV)
template <bool INV, class C> PPF_HD inline C sm_rot(C a) {
  return INV ? sm_mk<C>(-a.y, a.x) : sm_mk<C>(a.y, -a.x);
}

// the R-point DFT of v in place, forward e^{-2 pi i / R} or (INV) its conjugate
template <int R, bool INV, class C>
PPF_HD inline void smooth_butterfly(C (&v)[R]) {
  if constexpr (R == 2) {
    const C a = v[0], b = v[1];
    v[0] = sm_add(a, b);
    v[1] = sm_sub(a, b);
  } else if constexpr (R == 4) {
    const C t0 = sm_add(v[0], v[2]), t1 = sm_sub(v[0], v[2]);
    const C t2 = sm_add(v[1], v[3]), t3 = sm_rot<INV>(sm_sub(v[1], v[3]));
    v[0] = sm_add(t0, t2);
    v[1] = sm_add(t1, t3);
    v[2] = sm_sub(t0, t2);
    v[3] = sm_sub(t1, t3);
  } else if constexpr (R == 3) {
    constexpr double s3 = 0.86602540378443864676;  // sin(2 pi / 3)
    const C t = sm_add(v[1], v[2]), d = sm_sub(v[1], v[2]);
    const C m = sm_mk<C>(fma(-0.5, t.x, v[0].x), fma(-0.5, t.y, v[0].y));
    const C r = sm_rot<INV>(sm_mk<C>(s3 * d.x, s3 * d.y));
    v[0] = sm_add(v[0], t);
    v[1] = sm_add(m, r);
    v[2] = sm_sub(m, r);
  } else {
    static_assert(R == 5, "radix 2, 3, 4 or 5");
    constexpr double c1 = 0.30901699437494742410;   // cos(2 pi / 5)
    constexpr double c2 = -0.80901699437494742410;  // cos(4 pi / 5)
    constexpr double s1 = 0.95105651629515357212;   // sin(2 pi / 5)
    constexpr double s2 = 0.58778525229247312917;   // sin(4 pi / 5)
    const C a1 = sm_add(v[1], v[4]), b1 = sm_sub(v[1], v[4]);
    const C a2 = sm_add(v[2], v[3]), b2 = sm_sub(v[2], v[3]);
    const C m1 = sm_mk<C>(fma(c2, a2.x, fma(c1, a1.x, v[0].x)), fma(c2, a2.y, fma(c1, a1.y, v[0].y)));
    const C m2 = sm_mk<C>(fma(c1, a2.x, fma(c2, a1.x, v[0].x)), fma(c1, a2.y, fma(c2, a1.y, v[0].y)));
    const C n1 = sm_rot<INV>(sm_mk<C>(fma(s2, b2.x, s1 * b1.x), fma(s2, b2.y, s1 * b1.y)));
    const C n2 = sm_rot<INV>(sm_mk<C>(fma(-s1, b2.x, s2 * b1.x), fma(-s1, b2.y, s2 * b1.y)));
    v[0] = sm_add(v[0], sm_add(a1, a2));
    v[1] = sm_add(m1, n1);
    v[4] = sm_sub(m1, n1);
    v[2] = sm_add(m2, n2);
    v[3] = sm_sub(m2, n2);
  }
}

// One pass's geometry: N points, radix R, span Ns (R Ns divides N).
struct SmoothPass {
  int Q;           // N / R butterflies, inputs Q apart
  int Ns;
  int tstride;     // 2 N / (R Ns): the table step per unit of q k
  unsigned magic;  // smooth_magic(Ns)
  PPF_HD SmoothPass(int N, int R, int Ns_)
      : Q(N / R), Ns(Ns_), tstride(2 * (N / (R * Ns_))), magic(smooth_magic(Ns_)) {}
  PPF_HD int k(int j) const { return j - Ns * smooth_div(j, Ns, magic); }
};

// Butterfly j < Q of a pass: its R inputs from buf, twiddled, into v ...
template <int R, bool INV, class C>
PPF_HD inline void smooth_gather(const C* buf, const C* tw, const SmoothPass& ps, int j, C (&v)[R]) {
  const int tstep = ps.k(j) * ps.tstride;
  v[0] = buf[j];
  PPF_UNROLL
  for (int q = 1; q < R; ++q) {
    C w = tw[q * tstep];
    if (INV) w.y = -w.y;
    v[q] = sm_mul(buf[j + q * ps.Q], w);
  }
}

// ... and, once every butterfly of the pass has gathered, transformed and
// written to its outputs' places.
template <int R, bool INV, class C>
PPF_HD inline void smooth_scatter(C* buf, const SmoothPass& ps, int j, C (&v)[R]) {
  smooth_butterfly<R, INV>(v);
  const int k = ps.k(j);
  const int d = (j - k) * R + k;
  PPF_UNROLL
  for (int q = 0; q < R; ++q) buf[d + q * ps.Ns] = v[q];
}

// Bin k <= N of the real row's spectrum from the N-point transform Z of its
// packed samples (numpy rfft layout); w = tw[k] = e^{-2 pi i k / nbin}.
template <class C>
PPF_HD inline C smooth_rfft_post(const C* Z, int N, int k, C w) {
  const C zk = Z[k == N ? 0 : k];
  const C zn = Z[k == 0 ? 0 : N - k];
  const C zc = sm_mk<C>(zn.x, -zn.y);
  const C s = sm_add(zk, zc), dd = sm_sub(zk, zc);
  const C e = sm_mk<C>(0.5 * s.x, 0.5 * s.y);
  const C o = sm_mk<C>(0.5 * dd.y, -0.5 * dd.x);  // -i/2 (zk - zc)
  return sm_add(e, sm_mul(w, o));
}

// Packed spectrum Z_k (k < N) for the way back: irfft(X) = unpack(IFFT_N(Z))
// / N, from X_k and X_{N-k}; w = tw[k].  The caller has dropped the imaginary
// parts of X_0 and X_N (pocketfft c2r).
template <class C>
PPF_HD inline C smooth_irfft_pre(C xk, C xnk, C w) {
  const C xc = sm_mk<C>(xnk.x, -xnk.y);
  const C s = sm_add(xk, xc), dd = sm_sub(xk, xc);
  const C e = sm_mk<C>(0.5 * s.x, 0.5 * s.y);
  const C o = sm_mul(sm_mk<C>(0.5 * dd.x, 0.5 * dd.y), sm_mk<C>(w.x, -w.y));
  return sm_mk<C>(e.x - o.y, e.y + o.x);  // e + i o
}

}  // namespace ppf
