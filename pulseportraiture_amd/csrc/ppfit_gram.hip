// ppfit_gram.hip -- the PCA of portraits with more channels than bins
// (ppf_pca_gram_portraits): the nbin x nbin weighted covariance G = A^T A on
// the fp64 matrix cores, as the reference forms it (np.cov, pplib.py:1497-1534),
// then the Jacobi kernels of ppfit_pca.hip on G's nbin rows.
//
// A[n][i] = sqrt(w_n / fact) (port[n][i] - mean[i]) (0 where w_n = 0) is never
// stored: the row scale and the bin's mean are applied when a tile is loaded.
//
//   k_gram_mean    the weighted mean per bin and the row scales, in
//                  k_pca_center's order of sums (the mean is bitwise its);
//   k_gram_tiles   the 64 x 64 tiles of the lower triangle of G (a workgroup:
//                  2 x 2 of them), each summed over one slab of kGramSlab
//                  channels, into the workspace;
//   k_gram_reduce  the slabs added in slab order; the tile and its mirror
//                  written from the same value, so G is exactly symmetric;
//   k_gram_trace   trace(G), in a fixed order;
//   k_gram_null    the null-row threshold of a sweep from G's own error;
//   k_gram_sqrt    eigenvalue = |row| of the rotated G (k_pca_emit leaves
//                  |row|^2, the rows path's eigenvalue).
//
// G is symmetric positive semi-definite, so its right singular vectors are its
// eigenvectors and the norms of the rotated rows its eigenvalues.  The slab
// size is a compile-time constant and the slabs meet in a second launch in
// slab order: no atomics, and a portrait's G does not depend on the device,
// on the workspace limit or on what else shares the call.
#include "ppfit_kernels.hpp"

namespace ppf {

typedef double gram_f64x4 __attribute__((ext_vector_type(4)));

constexpr int kGramTile = 64;    // bins per side of a partial tile
constexpr int kGramBlock = 128;  // bins per side of a workgroup's block: 2 x 2 tiles
constexpr int kGramSlab = 256;   // channels per partial sum
constexpr int kGramKc = 16;      // channels staged in LDS at a time
constexpr int kGramLd = 144;     // LDS row stride in doubles: the two k of a half-wave in disjoint banks
constexpr int kGramMeanAhead = 16;  // channels whose loads k_gram_mean keeps in flight
constexpr int kGramLoads = kGramKc * kGramBlock / kBlock;  // values per thread, block and chunk
static_assert(kGramSlab % kGramKc == 0 && kGramKc % 4 == 0 && kGramBlock == 2 * kGramTile &&
                  kBlock == 2 * kGramBlock,
              "k_gram_tiles: four waves, one 64 x 64 tile each, chunks of whole MFMA steps");

// tiles of the lower triangle in nbin bins
inline int gram_ntile(int nbin) { return (nbin + kGramTile - 1) / kGramTile; }
inline int gram_npair(int nbin) { return gram_ntile(nbin) * (gram_ntile(nbin) + 1) / 2; }
inline int gram_nsuper(int nbin) {  // 128 x 128 blocks of the lower triangle
  const int nb = (nbin + kGramBlock - 1) / kGramBlock;
  return nb * (nb + 1) / 2;
}
inline int gram_nslab(int nchan) { return (nchan + kGramSlab - 1) / kGramSlab; }

// grid (ceil(nbin / 64), nport), 64 threads: a thread owns one bin of one
// portrait; the first block of a portrait also writes the row scales
__global__ __launch_bounds__(64) void k_gram_mean(const double* __restrict__ port,
                                                  const double* __restrict__ weights, int nchan,
                                                  int nbin, double* __restrict__ mean,
                                                  double* __restrict__ scale) {
  const int p = blockIdx.y, j = blockIdx.x * 64 + threadIdx.x;
  const double* w = weights + (size_t)p * nchan;
  double sw = 0.0, sw2 = 0.0;
  for (int n = 0; n < nchan; ++n) {
    const double wn = w[n];
    sw += wn;
    sw2 = fma(wn, wn, sw2);
  }
  const double fact = sw - sw2 / sw;
  if (blockIdx.x == 0)
    for (int n = threadIdx.x; n < nchan; n += 64) {
      const double wn = w[n];
      scale[(size_t)p * nchan + n] = wn != 0.0 ? sqrt(wn / fact) : 0.0;
    }
  if (j >= nbin) return;
  const double* x = port + (size_t)p * nchan * nbin + j;
  // the sum is k_pca_center's, term by term; the loads of kGramMeanAhead
  // channels are issued together (a bin's chain of additions has only
  // ceil(nbin / 64) waves per portrait to hide their latency)
  double s = 0.0;
  int n = 0;
  for (; n + kGramMeanAhead <= nchan; n += kGramMeanAhead) {
    double xv[kGramMeanAhead];
#pragma unroll
    for (int q = 0; q < kGramMeanAhead; ++q) xv[q] = x[(size_t)(n + q) * nbin];
#pragma unroll
    for (int q = 0; q < kGramMeanAhead; ++q) {
      const double wn = w[n + q];
      if (wn != 0.0) s += xv[q] * wn;
    }
  }
  for (; n < nchan; ++n) {
    const double wn = w[n];
    if (wn != 0.0) s += x[(size_t)n * nbin] * wn;
  }
  mean[(size_t)p * nbin + j] = s / sw;
}

// grid (nsuper, nslab, nport).  Workgroup: the 128 x 128 block (Ti, Tj), Tj <=
// Ti, of the lower triangle, i.e. 2 x 2 of the 64 x 64 tiles the partial sums
// are kept in; wave w the tile (2 Ti + (w >> 1), 2 Tj + (w & 1)) as 4 x 4 MFMA
// tiles.  Per step of 4 channels one v_mfma_f64_16x16x4 per MFMA tile: A
// operand = the I block's values (lane l: bin l & 15, channel l >> 4), B = the
// J block's; each value a lane reads from LDS feeds four MFMAs.  Channels
// past the slab's end and bins past nbin are staged as zeros.  A wave whose
// tile lies above the diagonal or past the last tile loads and idles.
__global__ __launch_bounds__(kBlock) void k_gram_tiles(const double* __restrict__ port,
                                                       const double* __restrict__ scale,
                                                       const double* __restrict__ mean, int nchan,
                                                       int nbin, int npair,
                                                       double* __restrict__ part) {
  __shared__ double sI[kGramKc * kGramLd], sJ[kGramKc * kGramLd];
  const int T = blockIdx.x, slab = blockIdx.y, p = blockIdx.z, nslab = gridDim.y;
  int Ti = 0;
  while ((Ti + 1) * (Ti + 2) / 2 <= T) ++Ti;
  const int Tj = T - Ti * (Ti + 1) / 2;
  const bool diag = Ti == Tj;
  const double* sB = diag ? sI : sJ;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int ri = lane & 15, kk = lane >> 4, wr = w >> 1, wc = w & 1;
  const int ti = 2 * Ti + wr, tj = 2 * Tj + wc;  // the wave's 64 x 64 tile
  const bool active = tj <= ti && ti * kGramTile < nbin;  // (then tj's bins start below nbin too)
  const int n0 = slab * kGramSlab, n1 = min(nchan, n0 + kGramSlab);
  // the loader: bin lb of both blocks, channels c0 + lc + 2 q
  const int lb = tid & (kGramBlock - 1), lc = tid / kGramBlock;
  const int bI = Ti * kGramBlock + lb, bJ = Tj * kGramBlock + lb;
  const bool okI = bI < nbin, okJ = !diag && bJ < nbin;
  const double muI = okI ? mean[(size_t)p * nbin + bI] : 0.0;
  const double muJ = okJ ? mean[(size_t)p * nbin + bJ] : 0.0;
  const double* x = port + (size_t)p * nchan * nbin;
  const double* sc = scale + (size_t)p * nchan;
  // fetch only loads (raw samples and row scales, channels past the slab's
  // end clamped to its last one and given scale 0), so that a chunk's loads
  // are all in flight under the MFMAs; stage() scales and centres them
  double ra[kGramLoads], rb[kGramLoads], rs[kGramLoads];
  auto fetch = [&](int c0) {
#pragma unroll
    for (int q = 0; q < kGramLoads; ++q) {
      const int n = c0 + lc + 2 * q, nn = min(n, n1 - 1);
      const double* row = x + (size_t)nn * nbin;
      const double s = sc[nn];
      rs[q] = n < n1 ? s : 0.0;
      ra[q] = okI ? row[bI] : 0.0;
      rb[q] = okJ ? row[bJ] : 0.0;
    }
  };
  auto stage = [&]() {
#pragma unroll
    for (int q = 0; q < kGramLoads; ++q) {
      const double s = rs[q];  // 0: a zero-weight row contributes nothing, whatever it holds
      sI[(lc + 2 * q) * kGramLd + lb] = (okI && s != 0.0) ? s * (ra[q] - muI) : 0.0;
      if (!diag) sJ[(lc + 2 * q) * kGramLd + lb] = (okJ && s != 0.0) ? s * (rb[q] - muJ) : 0.0;
    }
  };
  gram_f64x4 acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = (gram_f64x4){0.0, 0.0, 0.0, 0.0};
  fetch(n0);
  for (int c0 = n0; c0 < n1; c0 += kGramKc) {
    __syncthreads();  // the previous chunk has been consumed
    stage();
    __syncthreads();
    if (c0 + kGramKc < n1) fetch(c0 + kGramKc);  // in flight under the MFMAs
    if (active) {
#pragma unroll
      for (int st = 0; st < kGramKc / 4; ++st) {
        const double* rowI = sI + (4 * st + kk) * kGramLd + kGramTile * wr + ri;
        const double* rowJ = sB + (4 * st + kk) * kGramLd + kGramTile * wc + ri;
        double av[4], bv[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) {
          av[a] = rowI[16 * a];
          bv[a] = rowJ[16 * a];
        }
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
          for (int b = 0; b < 4; ++b)
            acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[a], bv[b], acc[a][b], 0, 0, 0);
      }
    }
  }
  if (!active) return;
  // lane l holds rows (l >> 4) + 4 r, column l & 15 of each MFMA tile
  const int t = ti * (ti + 1) / 2 + tj;
  double* out = part + (((size_t)p * nslab + slab) * npair + t) * (kGramTile * kGramTile);
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        out[(16 * a + kk + 4 * r) * kGramTile + 16 * b + ri] = acc[a][b][r];
}

// grid (npair, 16, nport): four rows of a tile per workgroup
__global__ __launch_bounds__(kBlock) void k_gram_reduce(const double* __restrict__ part, int nbin,
                                                        int nslab, double* __restrict__ G) {
  const int t = blockIdx.x, p = blockIdx.z, npair = gridDim.x;
  int ti = 0;
  while ((ti + 1) * (ti + 2) / 2 <= t) ++ti;
  const int tj = t - ti * (ti + 1) / 2;
  const int r = 4 * blockIdx.y + (threadIdx.x >> 6), c = threadIdx.x & 63;
  const int gi = ti * kGramTile + r, gj = tj * kGramTile + c;
  if (gi >= nbin || gj > gi) return;  // (gj <= gi < nbin)
  const double* src =
      part + ((size_t)p * nslab * npair + t) * (kGramTile * kGramTile) + r * kGramTile + c;
  double s = 0.0;
  for (int slab = 0; slab < nslab; ++slab)
    s += src[(size_t)slab * npair * (kGramTile * kGramTile)];
  double* g = G + (size_t)p * nbin * nbin;
  g[(size_t)gi * nbin + gj] = s;
  g[(size_t)gj * nbin + gi] = s;
}

// grid (nport)
__global__ __launch_bounds__(kBlock) void k_gram_trace(const double* __restrict__ G, int nbin,
                                                       double* __restrict__ trace) {
  __shared__ double red[kWaves];
  const int p = blockIdx.x;
  const double* g = G + (size_t)p * nbin * nbin;
  double s = 0.0;
  for (int j = threadIdx.x; j < nbin; j += kBlock) s += g[(size_t)j * nbin + j];
  s = block_sum(s, red);
  if (threadIdx.x == 0) trace[p] = s;
}

// ceil(nport / kBlock) blocks, after k_pca_sweep: an entry of G carries
// |error| <= nchan eps sqrt(G_ii G_jj), so |G - exact|_F <= nchan eps trace(G)
// and an eigenvalue that is exactly 0 arrives as a row of at most that norm.
// Such rows are null, beside the rows path's own floor (the rotations'
// rounding, eps sqrt(nbin) max|row|), which k_pca_sweep has just set.
__global__ __launch_bounds__(kBlock) void k_gram_null(PcaState* __restrict__ state,
                                                      const double* __restrict__ trace, int nchan,
                                                      int nport) {
  const int p = blockIdx.x * kBlock + threadIdx.x;
  if (p >= nport || state[p].done) return;
  const double tol = (double)nchan * kPcaEps * trace[p];
  state[p].null2 = fmax(state[p].null2, tol * tol);
}

// ceil(n / kBlock) blocks
__global__ __launch_bounds__(kBlock) void k_gram_sqrt(double* __restrict__ eigval, int n) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i < n) eigval[i] = sqrt(eigval[i]);
}

}  // namespace ppf
