// ppfit_fake.hip -- 16-bit PSRFITS samples from fp64 rows (ppf_pack_subints,
// the inverse of k_unpack) and the fake-pulsar generator (ppf_fake_subints:
// k_synth with polarisations, per-row amplitudes and per-channel noise), whose
// power-of-two kernel quantises the row it has just made in LDS.
#include "ppfit_kernels.hpp"

namespace ppf {

// Block-wide minimum and maximum; `red` is >= 2 kWaves doubles of LDS.  Every
// thread gets them (threads without a sample pass +inf / -inf).
__device__ __forceinline__ void block_minmax(double& lo, double& hi, double* red) {
  lo = -wave_max(-lo);
  hi = wave_max(hi);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0) { red[w] = lo; red[kWaves + w] = hi; }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < kWaves; ++i) {
    lo = fmin(lo, red[i]);
    hi = fmax(hi, red[kWaves + i]);
  }
  __syncthreads();
}

// The quantiser of a row with exact minimum lo and maximum hi (ppfit.h,
// ppf_pack_subints): offs the float32 nearest the mid-range, scl the smallest
// float32 >= the larger distance from offs to an extreme over 32767, so that
// rint((x - offs) / scl) is within +-32767 for every sample without a clamp.
// A constant row takes scl = 1.
struct RowQuant {
  double scl, offs;
  __device__ __forceinline__ RowQuant(double lo, double hi) {
    offs = (double)(float)(0.5 * (lo + hi));
    scl = 1.0;
    if (lo == hi) return;
    const double w = fmax(hi - offs, offs - lo) / 32767.0;
    float f = (float)w;
    if ((double)f < w) f = __uint_as_float(__float_as_uint(f) + 1u);  // next float32 up (f >= 0)
    scl = (double)f;
  }
  __device__ __forceinline__ short operator()(double x) const {
    return (short)(int)rint((x - offs) / scl);
  }
};

__device__ __forceinline__ bool not_finite(double x) { return !(fabs(x) <= 1.7976931348623157e308); }

// One workgroup per row [nbin] of data: a pass for the extremes, one for the
// samples (the second read of a row of at most 64 KB comes from cache).  A
// row with a non-finite sample sets *bad and is stored as zeros.
__global__ __launch_bounds__(kBlock) void k_pack(const double* __restrict__ data, int nbin,
                                                 short* __restrict__ raw,
                                                 double* __restrict__ scl,
                                                 double* __restrict__ offs,
                                                 int* __restrict__ bad) {
  __shared__ double red[2 * kWaves];
  const size_t row = blockIdx.x;
  const int tid = threadIdx.x;
  const double* __restrict__ x = data + row * nbin;
  short* __restrict__ o = raw + row * nbin;
  const bool pairs = !(nbin & 1);  // rows of even length: 16-byte loads, 4-byte stores
  double lo = INFINITY, hi = -INFINITY;
  int nf = 0;
  if (pairs) {
    const double2* __restrict__ x2 = reinterpret_cast<const double2*>(x);
    for (int j = tid; 2 * j < nbin; j += kBlock) {
      const double2 v = x2[j];
      nf |= not_finite(v.x) | not_finite(v.y);
      lo = fmin(lo, fmin(v.x, v.y));
      hi = fmax(hi, fmax(v.x, v.y));
    }
  } else {
    for (int j = tid; j < nbin; j += kBlock) {
      const double v = x[j];
      nf |= not_finite(v);
      lo = fmin(lo, v);
      hi = fmax(hi, v);
    }
  }
  nf = __syncthreads_or(nf);
  if (nf) { lo = 0.0; hi = 0.0; }
  block_minmax(lo, hi, red);
  const RowQuant q(lo, hi);
  if (tid == 0) {
    scl[row] = q.scl;
    offs[row] = q.offs;
    if (nf) *bad = 1;
  }
  if (pairs) {
    const double2* __restrict__ x2 = reinterpret_cast<const double2*>(x);
    short2* __restrict__ o2 = reinterpret_cast<short2*>(o);
    for (int j = tid; 2 * j < nbin; j += kBlock) {
      const double2 v = x2[j];
      o2[j] = nf ? make_short2(0, 0) : make_short2(q(v.x), q(v.y));
    }
  } else {
    for (int j = tid; j < nbin; j += kBlock) o[j] = nf ? (short)0 : q(x[j]);
  }
}

// Sample pair j of the row (subint gs, channel word cw): amp * v + sigma * the
// pair's Philox normals -- k_synth's epilogue when amp = 1.
struct FakeEpi {
  double amp, sigma;
  uint64_t seed, gs;
  uint32_t cw;
  __device__ __forceinline__ bool active() const { return true; }  // amp
  template <class V>
  __device__ __forceinline__ double2 operator()(int j, V v0) const {
    double2 v = v0;
    v.x *= amp;
    v.y *= amp;
    if (sigma != 0.0) {
      u32x4 ctr;
      ctr.v[0] = (uint32_t)j;
      ctr.v[1] = cw;
      ctr.v[2] = (uint32_t)gs;
      ctr.v[3] = (uint32_t)(gs >> 32);
      const double2 z = philox_normal2(ctr, seed);
      v.x = fma(sigma, z.x, v.x);
      v.y = fma(sigma, z.y, v.y);
    }
    return v;
  }
};

// the row of workgroup `row` = (s * npol + p) * nchan + n
__device__ __forceinline__ FakeEpi fake_row(const FakeArgs& a, size_t row, int* n_out,
                                            double* phase_out) {
  const int n = (int)(row % a.nchan);
  const size_t sp = row / a.nchan;
  const int p = (int)(sp % a.npol);
  const size_t s = sp / a.npol;
  *n_out = n;
  *phase_out = a.phase[s * a.nchan + n];
  FakeEpi e;
  e.amp = a.amp[s * a.nchan + n];
  e.sigma = a.sigma[n];
  e.seed = a.seed;
  e.gs = (uint64_t)((int64_t)s + a.sub0);
  e.cw = (uint32_t)n + (uint32_t)a.nchan * (uint32_t)p;
  return e;
}

// data[s][p][n] = amp[s][n] irfft(Mfull_n e^{2 pi i k phase[s][n]}) + sigma[n] N(0,1), one
// workgroup per row.  PACK (RowPow2 only; the host packs RowAny's fp64 rows
// with k_pack): the row stays in LDS after the transform; its extremes, the
// quantiser and the int16 stores follow (no fp64 row in HBM).
template <class Row, bool PACK>
__global__ __launch_bounds__(kBlock) void k_fake(FakeArgs a, const double2* __restrict__ tw,
                                                 Row rw) {
  __shared__ typename Row::template Lds<kLdsSpec> sm;
  __shared__ double red[2 * kWaves];
  typename Row::Dev t(rw, sm, tw);
  const size_t row = blockIdx.x;
  const int tid = threadIdx.x;
  int n;
  double ph;
  const FakeEpi epi = fake_row(a, row, &n, &ph);
  typename Row::Own xs(t.spec);
  t.for_bins([&](int i, int k) {
    xs.at(i, k) = cmul(a.M[(size_t)n * a.NHP + k], turn_phasor((double)k, ph));
  });
  if constexpr (!PACK) {
    t.inverse(xs, a.data + row * t.nbin(), epi);
  } else {
    constexpr int N = Row::N;
    double2* buf = t.buf;
    c2r_in_lds<Row::kLogN>(buf, xs.v, tw);
    const double inv = 1.0 / (double)N;
    double lo = INFINITY, hi = -INFINITY;
    int nf = 0;
    for (int j = tid; j < N; j += kBlock) {
      const double2 v = epi(j, cscale(buf[j], inv));
      buf[j] = v;
      nf |= not_finite(v.x) | not_finite(v.y);
      lo = fmin(lo, fmin(v.x, v.y));
      hi = fmax(hi, fmax(v.x, v.y));
    }
    nf = __syncthreads_or(nf);  // every buf[j] is final past this barrier
    if (nf) { lo = 0.0; hi = 0.0; }
    block_minmax(lo, hi, red);
    const RowQuant q(lo, hi);
    if (tid == 0) {
      a.scl[row] = q.scl;
      a.offs[row] = q.offs;
      if (nf) *a.bad = 1;
    }
    // two sample pairs (8 bytes of int16) per thread and store
    short4* __restrict__ o4 = reinterpret_cast<short4*>(a.raw + row * 2 * N);
    for (int j = 2 * tid; j < N; j += 2 * kBlock) {
      const double2 u = buf[j], v = buf[j + 1];
      o4[j >> 1] = nf ? make_short4(0, 0, 0, 0) : make_short4(q(u.x), q(u.y), q(v.x), q(v.y));
    }
  }
}

#define PPF_INST_FAKE(L)                                                                     \
  template __global__ void k_fake<RowPow2<L>, false>(FakeArgs, const double2*, RowPow2<L>);  \
  template __global__ void k_fake<RowPow2<L>, true>(FakeArgs, const double2*, RowPow2<L>);
PPF_INST_FAKE(5)
PPF_INST_FAKE(6)
PPF_INST_FAKE(7)
PPF_INST_FAKE(8)
PPF_INST_FAKE(9)
PPF_INST_FAKE(10)
PPF_INST_FAKE(11)
PPF_INST_FAKE(12)
template __global__ void k_fake<RowAny, false>(FakeArgs, const double2*, RowAny);
template __global__ void k_fake<RowSmooth<1024>, false>(FakeArgs, const double2*, RowSmooth<1024>);
template __global__ void k_fake<RowSmooth<4096>, false>(FakeArgs, const double2*, RowSmooth<4096>);

}  // namespace ppf
