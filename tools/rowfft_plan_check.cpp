// rowfft_plan_check.cpp -- the plan and the passes of the mixed-radix row FFT
// (csrc/ppfit_smoothfft.hpp), run on the host for every eligible length, as a
// stand-alone program (no GPU, no HIP):
//
//   g++ -std=c++17 -O2 -Ipulseportraiture_amd/csrc tools/rowfft_plan_check.cpp -o rowfft_plan_check
//   ./rowfft_plan_check            (add -g -fsanitize=address,undefined to check the indices too)
//
// For every nbin in [16, 8192] that row_kind() calls smooth it transforms a
// seeded row forwards (pack, passes, smooth_rfft_post) and a spectrum back
// (smooth_irfft_pre, passes, unpack) with the very functions the kernels call,
// the workgroup's threads played by a loop and the twiddle table made from
// cos / sin in double, and compares both with a direct DFT accumulated in long
// double.  The bar is 1e-12 of the largest |value| of the spectrum or row,
// absolute.  It also checks that every table and buffer index stays inside its
// array, that the radices multiply to N, that the per-thread chunks fit the
// size class's register arrays, and the predicate's table of include/ppfit.h.
// Exit status 0 and "ok <lengths> <worst forward> <worst inverse>".
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ppfit_smoothfft.hpp"

using namespace ppf;

namespace {

struct Cx { double x, y; };
constexpr int kBlock = 256;

#define CHECK(cond)                                                                     \
  do {                                                                                  \
    if (!(cond)) {                                                                      \
      fprintf(stderr, "%s:%d: nbin %d: %s failed\n", __FILE__, __LINE__, nbin, #cond);  \
      return 1;                                                                         \
    }                                                                                   \
  } while (0)

double uniform(unsigned long long& s) {  // splitmix64 -> [-1, 1)
  s += 0x9E3779B97F4A7C15ull;
  unsigned long long z = s;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  return (double)(z >> 11) * (2.0 / 9007199254740992.0) - 1.0;
}

template <int R, bool INV>
bool run_pass(Cx* buf, const Cx* tw, int N, int Ns, int maxn, int nbin, int* worst_tw) {
  const SmoothPass ps(N, R, Ns);
  const int chunks = smooth_chunks(maxn, R);
  if ((ps.Q + kBlock - 1) / kBlock > chunks) return false;  // the register arrays' bound
  std::vector<Cx> regs((size_t)kBlock * chunks * R);
  for (int j = 0; j < ps.Q; ++j) {  // what smooth_gather will index
    const int k = j % Ns;
    if (ps.k(j) != k) return false;
    const int top = (R - 1) * k * ps.tstride;
    if (top >= nbin || j + (R - 1) * ps.Q >= N) return false;
    if (top > *worst_tw) *worst_tw = top;
    if ((j - k) * R + k + (R - 1) * Ns >= N) return false;
  }
  for (int tid = 0; tid < kBlock; ++tid)
    for (int c = 0; c < chunks; ++c) {
      const int j = tid + c * kBlock;
      if (j < ps.Q) smooth_gather<R, INV>(buf, tw, ps, j, *reinterpret_cast<Cx(*)[R]>(&regs[((size_t)tid * chunks + c) * R]));
    }
  // (the block's barrier)
  for (int tid = 0; tid < kBlock; ++tid)
    for (int c = 0; c < chunks; ++c) {
      const int j = tid + c * kBlock;
      if (j < ps.Q) smooth_scatter<R, INV>(buf, ps, j, *reinterpret_cast<Cx(*)[R]>(&regs[((size_t)tid * chunks + c) * R]));
    }
  return true;
}

template <bool INV>
bool run_fft(Cx* buf, const Cx* tw, const SmoothPlan& p, int nbin, int* worst_tw) {
  const int maxn = smooth_class(p.n);
  int Ns = 1;
  for (int s = 0; s < p.npass; ++s) {
    const int r = p.radix(s);
    bool ok = false;
    switch (r) {
      case 2: ok = run_pass<2, INV>(buf, tw, p.n, Ns, maxn, nbin, worst_tw); break;
      case 3: ok = run_pass<3, INV>(buf, tw, p.n, Ns, maxn, nbin, worst_tw); break;
      case 4: ok = run_pass<4, INV>(buf, tw, p.n, Ns, maxn, nbin, worst_tw); break;
      case 5: ok = run_pass<5, INV>(buf, tw, p.n, Ns, maxn, nbin, worst_tw); break;
      default: break;
    }
    if (!ok) return false;
    Ns *= r;
  }
  return Ns == p.n;
}

int predicate_table() {
  int nbin = 0;
  for (int v : {96, 100, 768, 1000, 1536, 2000, 3000, 6144, 8000, 8100}) {
    nbin = v;
    CHECK(row_kind(v, true) == kRowSmooth);
    CHECK(row_kind(v, false) == kRowDirect);
  }
  for (nbin = 17; nbin < 8192; nbin += 2) CHECK(row_kind(nbin, true) == kRowDirect);
  nbin = 8190;
  CHECK(row_kind(nbin, true) == kRowDirect);
  for (nbin = 64; nbin <= 8192; nbin *= 2) {
    CHECK(row_kind(nbin, true) == kRowPow2);
    CHECK(row_kind(nbin, false) == kRowPow2);
  }
  return 0;
}

}  // namespace

int main() {
  if (predicate_table()) return 1;
  const long double pi = acosl(-1.0L);
  double worst_f = 0.0, worst_i = 0.0;
  int count = 0;
  for (int nbin = 16; nbin <= 8192; ++nbin) {
    if (row_kind(nbin, true) != kRowSmooth) continue;
    ++count;
    SmoothPlan p;
    CHECK(smooth_plan(nbin, &p));
    CHECK(p.n == nbin / 2 && p.npass >= 1 && p.npass <= kSmoothMaxPass);
    const int N = p.n, NH = N + 1;
    // the table the device holds (k_twiddles), and the reference's in long double
    std::vector<Cx> tw(nbin);
    std::vector<long double> rc(nbin), rs(nbin);
    for (int m = 0; m < nbin; ++m) {
      const double a = 2.0 * M_PI * (double)m / (double)nbin;
      tw[m] = Cx{cos(a), -sin(a)};
      const long double b = 2.0L * pi * (long double)m / (long double)nbin;
      rc[m] = cosl(b);
      rs[m] = sinl(b);
    }
    unsigned long long seed = 0x5eedULL * (unsigned long long)nbin;
    std::vector<double> x(nbin);
    for (double& v : x) v = uniform(seed);

    // forward: pack, passes, post
    std::vector<Cx> buf(N + 1);
    for (int j = 0; j < N; ++j) buf[j] = Cx{x[2 * j], x[2 * j + 1]};
    int worst_tw = 0;
    CHECK((run_fft<false>(buf.data(), tw.data(), p, nbin, &worst_tw)));
    std::vector<Cx> X(NH);
    for (int k = 0; k < NH; ++k) X[k] = smooth_rfft_post(buf.data(), N, k, tw[k]);
    long double big = 0.0L, err = 0.0L;
    std::vector<Cx> Xref(NH);
    for (int k = 0; k < NH; ++k) {
      long double re = 0.0L, im = 0.0L;
      int idx = 0;
      for (int m = 0; m < nbin; ++m) {
        re += (long double)x[m] * rc[idx];
        im -= (long double)x[m] * rs[idx];
        idx += k;
        if (idx >= nbin) idx -= nbin;
      }
      Xref[k] = Cx{(double)re, (double)im};
      big = fmaxl(big, hypotl(re, im));
      err = fmaxl(err, fmaxl(fabsl(re - X[k].x), fabsl(im - X[k].y)));
    }
    const double ef = (double)(err / big);
    CHECK(ef <= 1e-12);
    if (ef > worst_f) worst_f = ef;

    // the way back, from the reference's spectrum: pre, passes, unpack / N
    std::vector<Cx> S = Xref;
    S[0].y = 0.0;
    S[N].y = 0.0;
    for (int k = 0; k < N; ++k) buf[k] = smooth_irfft_pre(S[k], S[N - k], tw[k]);
    CHECK((run_fft<true>(buf.data(), tw.data(), p, nbin, &worst_tw)));
    CHECK(worst_tw < nbin);
    big = 0.0L;
    err = 0.0L;
    for (int m = 0; m < nbin; ++m) {
      // irfft(S, n = nbin)_m = (S_0 + (-1)^m S_N + 2 sum_{0<k<N} Re(S_k e^{+2 pi i k m / nbin})) / nbin
      long double acc = (long double)S[0].x + ((m & 1) ? -(long double)S[N].x : (long double)S[N].x);
      int idx = m % nbin;
      for (int k = 1; k < N; ++k) {
        acc += 2.0L * ((long double)S[k].x * rc[idx] - (long double)S[k].y * rs[idx]);
        idx += m;
        if (idx >= nbin) idx -= nbin;
      }
      acc /= (long double)nbin;
      const Cx z = buf[m / 2];
      const double got = ((m & 1) ? z.y : z.x) * (1.0 / (double)N);
      big = fmaxl(big, fabsl(acc));
      err = fmaxl(err, fabsl(acc - got));
    }
    const double ei = (double)(err / big);
    CHECK(ei <= 1e-12);
    if (ei > worst_i) worst_i = ei;
  }
  printf("ok %d %.3g %.3g\n", count, worst_f, worst_i);
  return 0;
}
