// ppfit_pca.hip -- batched principal components of portraits on the device
// (ppspline model building; pplib.pca, pplib.py:1497-1534, and
// reconstruct_portrait, pplib.py:1536-1553).
//
// The reference subtracts the weighted mean profile, forms
// np.cov(delta.T, aweights=w, ddof=1) -- centred by the weighted mean, divided
// by fact = sum w - sum w^2 / sum w -- and takes eigh of that nbin x nbin
// matrix.  With A[n] = sqrt(w_n / fact) (port[n] - mean) the covariance is
// A^T A: its eigenvectors are A's right singular vectors and its eigenvalues
// the squared singular values.  They come from a one-sided (Hestenes) Jacobi
// on the rows of A in fp64: row pairs are rotated until all rows are mutually
// orthogonal, then eigenvector = row / |row| and eigenvalue = |row|^2.  No
// nbin x nbin matrix and no rotation accumulator exist.
//
//   k_pca_center  the weighted mean per bin (channels in order) and A;
//   k_pca_norms   |row|^2 of every row;
//   k_pca_sweep   per portrait, between sweeps: converged (the last sweep
//                 rotated nothing) / out of sweeps / the null-row threshold
//                 of the next sweep;
//   k_pca_step    one round of a round-robin tournament: ceil(m / 2) disjoint
//                 row pairs (a bye when m is odd), one workgroup per pair and
//                 portrait; three dot products, then the rotation;
//   k_pca_rank    stable order of the rows by (|row|^2 descending, index);
//   k_pca_emit    eigenvalue, normalised row and its sign per component;
//   k_pca_project projections of (port - mean) on the vectors and, optionally,
//                 the reconstructed portrait.
//
// Every sum runs in a fixed order (a thread's strided partial, then
// block_sum) and a portrait's launches depend on no other portrait, so the
// results are bitwise reproducible and independent of what else shares the
// call.  Rounds are plain launches on the context stream: no grid barrier.
#include "ppfit_kernels.hpp"

namespace ppf {

constexpr double kPcaEps = 2.220446049250313e-16;

// a = x.x, b = y.y, c = x.y; every thread gets them
__device__ __forceinline__ void pca_dots(const double* __restrict__ x, const double* __restrict__ y,
                                         int nbin, double* red, double& a, double& b, double& c) {
  double sa = 0.0, sb = 0.0, sc = 0.0;
  for (int j = threadIdx.x; j < nbin; j += kBlock) {
    const double xv = x[j], yv = y[j];
    sa = fma(xv, xv, sa);
    sb = fma(yv, yv, sb);
    sc = fma(xv, yv, sc);
  }
  a = block_sum(sa, red);
  b = block_sum(sb, red);
  c = block_sum(sc, red);
}

// grid (ceil(nbin / kBlock), nport): a thread owns one bin of one portrait
__global__ __launch_bounds__(kBlock) void k_pca_center(const double* __restrict__ port,
                                                       const double* __restrict__ weights,
                                                       int nchan, int nbin,
                                                       double* __restrict__ mean,
                                                       double* __restrict__ A) {
  const int p = blockIdx.y, j = blockIdx.x * kBlock + threadIdx.x;
  const double* w = weights + (size_t)p * nchan;
  double sw = 0.0, sw2 = 0.0;
  for (int n = 0; n < nchan; ++n) {
    const double wn = w[n];
    sw += wn;
    sw2 = fma(wn, wn, sw2);
  }
  if (j >= nbin) return;
  const double fact = sw - sw2 / sw;
  const double* x = port + (size_t)p * nchan * nbin + j;
  double s = 0.0;
  for (int n = 0; n < nchan; ++n) {
    const double wn = w[n];
    if (wn != 0.0) s += x[(size_t)n * nbin] * wn;
  }
  const double mu = s / sw;
  mean[(size_t)p * nbin + j] = mu;
  double* a = A + (size_t)p * nchan * nbin + j;
  for (int n = 0; n < nchan; ++n) {
    const double wn = w[n];
    a[(size_t)n * nbin] = wn != 0.0 ? sqrt(wn / fact) * (x[(size_t)n * nbin] - mu) : 0.0;
  }
}

// grid (m, nport)
__global__ __launch_bounds__(kBlock) void k_pca_norms(const double* __restrict__ A, int m, int nbin,
                                                      double* __restrict__ norm2) {
  __shared__ double red[kWaves];
  const int r = blockIdx.x, p = blockIdx.y;
  const double* x = A + ((size_t)p * m + r) * nbin;
  double s = 0.0;
  for (int j = threadIdx.x; j < nbin; j += kBlock) s = fma(x[j], x[j], s);
  s = block_sum(s, red);
  if (threadIdx.x == 0) norm2[(size_t)p * m + r] = s;
}

// grid (nport): the state of a portrait before sweep number `sweep`
__global__ __launch_bounds__(kBlock) void k_pca_sweep(PcaState* __restrict__ state,
                                                      const double* __restrict__ norm2, int m,
                                                      int nbin, int sweep, int max_sweeps) {
  __shared__ double red[kWaves];
  const int p = blockIdx.x;
  PcaState* st = state + p;
  if (st->done) return;  // (no thread writes it before the barrier below)
  double mx = 0.0;
  for (int r = threadIdx.x; r < m; r += kBlock) mx = fmax(mx, norm2[(size_t)p * m + r]);
  mx = wave_max(mx);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
  __syncthreads();
  if (threadIdx.x != 0) return;
  for (int i = 0; i < kWaves; ++i) mx = fmax(mx, red[i]);
  if (sweep > 0 && st->rot == 0) {
    st->done = 1;
    st->converged = 1;
  } else if (sweep >= max_sweeps) {
    st->done = 1;
    st->converged = 0;
  } else {
    // rows at or below this |row|^2 are null (rank-deficient input): they
    // cannot be made orthogonal to rounding and are left alone
    st->null2 = kPcaEps * kPcaEps * (double)nbin * mx;
    st->rot = 0;
    st->sweeps = sweep + 1;
  }
}

// grid (M / 2, nport), M = m rounded up to even: round `round` (0 .. M - 2)
// of the circle method; index M - 1 sits still, the others turn.
__global__ __launch_bounds__(kBlock) void k_pca_step(double* __restrict__ A,
                                                     PcaState* __restrict__ state, int m, int M,
                                                     int nbin, int round) {
  __shared__ double red[kWaves];
  const int k = blockIdx.x, p = blockIdx.y;
  PcaState* st = state + p;
  if (st->done) return;
  const int M1 = M - 1;
  const int i0 = k == 0 ? M1 : (round + k) % M1;
  const int j0 = k == 0 ? round : (round - k + M1) % M1;
  const int lo = min(i0, j0), hi = max(i0, j0);
  if (hi >= m) return;  // the bye of an odd m
  double* x = A + ((size_t)p * m + lo) * nbin;
  double* y = A + ((size_t)p * m + hi) * nbin;
  double a, b, c;
  pca_dots(x, y, nbin, red, a, b, c);
  const double null2 = st->null2;
  if (a <= null2 || b <= null2) return;
  if (!(fabs(c) > 4.0 * kPcaEps * sqrt(a) * sqrt(b))) return;
  const double zeta = (b - a) / (2.0 * c);
  const double t = (zeta < 0.0 ? -1.0 : 1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
  const double cs = 1.0 / sqrt(1.0 + t * t), sn = cs * t;
  for (int j = threadIdx.x; j < nbin; j += kBlock) {
    const double xv = x[j], yv = y[j];
    x[j] = cs * xv - sn * yv;
    y[j] = sn * xv + cs * yv;
  }
  if (threadIdx.x == 0) atomicAdd(&st->rot, 1);
}

// grid (nport), m doubles of dynamic LDS: order[p][rank] = row, for the
// ncomp leading rows by (|row|^2 descending, row index)
__global__ __launch_bounds__(kBlock) void k_pca_rank(const double* __restrict__ norm2, int m,
                                                     int ncomp, int* __restrict__ order) {
  extern __shared__ double s_n[];
  const int p = blockIdx.x;
  for (int r = threadIdx.x; r < m; r += kBlock) s_n[r] = norm2[(size_t)p * m + r];
  __syncthreads();
  for (int r = threadIdx.x; r < m; r += kBlock) {
    const double v = s_n[r];
    int rank = 0;
    for (int s = 0; s < m; ++s) {
      const double u = s_n[s];
      rank += (u > v || (u == v && s < r)) ? 1 : 0;
    }
    if (rank < ncomp) order[(size_t)p * ncomp + rank] = r;
  }
}

// grid (ncomp, nport): component e of portrait p.  The vector's
// largest-magnitude component (the first such) is made positive.
__global__ __launch_bounds__(kBlock) void k_pca_emit(const double* __restrict__ A,
                                                     const double* __restrict__ norm2,
                                                     const int* __restrict__ order,
                                                     const PcaState* __restrict__ state, int m,
                                                     int nbin, int ncomp,
                                                     double* __restrict__ eigval,
                                                     double* __restrict__ eigvec,
                                                     int* __restrict__ info) {
  __shared__ double s_v[kBlock];
  __shared__ int s_i[kBlock];
  const int e = blockIdx.x, p = blockIdx.y, tid = threadIdx.x;
  const int r = order[(size_t)p * ncomp + e];
  const double n2 = norm2[(size_t)p * m + r];
  const double nrm = sqrt(n2);
  const double* x = A + ((size_t)p * m + r) * nbin;
  double* v = eigvec + ((size_t)p * ncomp + e) * nbin;
  double best = -1.0;
  int at = nbin;
  for (int j = tid; j < nbin; j += kBlock) {
    const double q = nrm > 0.0 ? fabs(x[j] / nrm) : 0.0;
    if (q > best) { best = q; at = j; }
  }
  s_v[tid] = best;
  s_i[tid] = at;
  __syncthreads();
  for (int h = kBlock / 2; h > 0; h >>= 1) {
    if (tid < h) {
      const double u = s_v[tid + h];
      const int ui = s_i[tid + h];
      if (u > s_v[tid] || (u == s_v[tid] && ui < s_i[tid])) { s_v[tid] = u; s_i[tid] = ui; }
    }
    __syncthreads();
  }
  const int jm = s_i[0] < nbin ? s_i[0] : 0;  // (a row of NaNs has no maximum)
  const double sgn = x[jm] < 0.0 ? -1.0 : 1.0;
  for (int j = tid; j < nbin; j += kBlock) v[j] = nrm > 0.0 ? sgn * (x[j] / nrm) : 0.0;
  if (tid == 0) {
    eigval[(size_t)p * ncomp + e] = n2;
    if (e == 0) {
      info[2 * p] = state[p].sweeps;
      info[2 * p + 1] = state[p].converged;
    }
  }
}

// grid (nchan, nport), ncomp doubles of dynamic LDS: proj[n][e] =
// (port[n] - mean) . v_e, reconst[n] = sum_e proj[n][e] v_e + mean
__global__ __launch_bounds__(kBlock) void k_pca_project(const double* __restrict__ port,
                                                        const double* __restrict__ mean,
                                                        const double* __restrict__ eigvec,
                                                        int nchan, int nbin, int ncomp,
                                                        double* __restrict__ proj,
                                                        double* __restrict__ reconst) {
  extern __shared__ double s_p[];
  __shared__ double red[kWaves];
  const int n = blockIdx.x, p = blockIdx.y, tid = threadIdx.x;
  const double* x = port + ((size_t)p * nchan + n) * nbin;
  const double* mu = mean + (size_t)p * nbin;
  const double* V = eigvec + (size_t)p * ncomp * nbin;
  for (int e = 0; e < ncomp; ++e) {
    const double* v = V + (size_t)e * nbin;
    double s = 0.0;
    for (int j = tid; j < nbin; j += kBlock) s = fma(x[j] - mu[j], v[j], s);
    s = block_sum(s, red);
    if (tid == 0) {
      proj[((size_t)p * nchan + n) * ncomp + e] = s;
      s_p[e] = s;
    }
  }
  if (!reconst) return;
  __syncthreads();
  double* out = reconst + ((size_t)p * nchan + n) * nbin;
  for (int j = tid; j < nbin; j += kBlock) {
    double s = 0.0;
    for (int e = 0; e < ncomp; ++e) s = fma(s_p[e], V[(size_t)e * nbin + j], s);
    out[j] = s + mu[j];
  }
}

}  // namespace ppf
