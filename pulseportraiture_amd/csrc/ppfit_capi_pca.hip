// ppfit_capi_pca.hip -- the PCA entry points of libppfit: the Jacobi on the
// portraits' rows (ppfit_pca.hip), on their Gram matrices (ppfit_gram.hip),
// and the projection.
#include "ppfit_host.hpp"

namespace {

// The weights [nport][nchan] are checked on the host: fact = sum w -
// sum w^2 / sum w must be > 0.
int pca_check_weights(ppf_ctx* ctx, const double* weights, int nport, int nchan) {
  std::vector<double> hw;
  if (int r = fetch(ctx, weights, (size_t)nport * nchan, hw)) return r;
  for (int p = 0; p < nport; ++p) {
    int npos = 0;
    for (int n = 0; n < nchan; ++n) {
      const double w = hw[(size_t)p * nchan + n];
      if (!std::isfinite(w) || w < 0.0)
        return fail(ctx, PPF_ERR_INVALID, "portrait %d: weight %d is %g (need finite, >= 0)", p, n,
                    w);
      npos += w > 0.0;
    }
    if (npos < 2)
      return fail(ctx, PPF_ERR_INVALID, "portrait %d: %d positive weights (need at least 2)", p,
                  npos);
  }
  return PPF_OK;
}

// What the Jacobi works on, for a chunk of portraits: m rows of nbin each per
// portrait (the centred portrait, or its Gram matrix), |row|^2, the state and
// the order of the ncomp leading rows.
struct PcaRows {
  double* A;
  double* norm2;
  PcaState* state;
  int* order;
  int m, nbin, ncomp;
};

int pca_reset(ppf_ctx* ctx, const PcaRows& w, int np) {
  HIPCHK(ctx, hipMemsetAsync(w.state, 0, (size_t)np * sizeof(PcaState), ctx->stream));
  HIPCHK(ctx, hipMemsetAsync(w.order, 0, (size_t)np * w.ncomp * sizeof(int), ctx->stream));
  return PPF_OK;
}

// The sweeps of np portraits.  The host reads the portraits' states once per
// sweep and stops when every one is done (converged, or kPcaMaxSweeps sweeps
// made).  after_sweep: further launches of the sweep's bracket.
template <typename F>
int pca_jacobi(ppf_ctx* ctx, const PcaRows& w, int np, F&& after_sweep) {
  const int m = w.m, M = (m + 1) & ~1, nbin = w.nbin;
  std::vector<PcaState> hs;
  for (int sweep = 0; sweep <= kPcaMaxSweeps; ++sweep) {
    if (int r = timed(ctx, PPF_K_PCA, [&] {
          hipLaunchKernelGGL(k_pca_norms, dim3(m, np), dim3(kBlock), 0, ctx->stream, w.A, m, nbin,
                             w.norm2);
          hipLaunchKernelGGL(k_pca_sweep, dim3(np), dim3(kBlock), 0, ctx->stream, w.state, w.norm2,
                             m, nbin, sweep, kPcaMaxSweeps);
          after_sweep();
        }))
      return r;
    bool all_done;
    if (int r = poll_done(ctx, w.state, np, hs, &all_done)) return r;
    if (all_done) break;
    if (int r = timed(ctx, PPF_K_PCA, [&] {
          for (int round = 0; round < M - 1; ++round)
            hipLaunchKernelGGL(k_pca_step, dim3(M / 2, np), dim3(kBlock), 0, ctx->stream, w.A,
                               w.state, m, M, nbin, round);
        }))
      return r;
  }
  return PPF_OK;
}

// The ncomp leading rows of np portraits into the results of portrait p0 ..
// (norm2 holds the final rows' norms: a done portrait is not rotated again).
// after_emit: further launches of the same bracket.
template <typename F>
int pca_emit(ppf_ctx* ctx, const PcaRows& w, int np, int64_t p0, double* eigval, double* eigvec,
             int32_t* info, F&& after_emit) {
  const int m = w.m, nbin = w.nbin, ncomp = w.ncomp;
  return timed(ctx, PPF_K_PCA, [&] {
    hipLaunchKernelGGL(k_pca_rank, dim3(np), dim3(kBlock), (size_t)m * sizeof(double), ctx->stream,
                       w.norm2, m, ncomp, w.order);
    hipLaunchKernelGGL(k_pca_emit, dim3(ncomp, np), dim3(kBlock), 0, ctx->stream, w.A, w.norm2,
                       w.order, w.state, m, nbin, ncomp, eigval + (size_t)p0 * ncomp,
                       eigvec + (size_t)p0 * ncomp * nbin, info + (size_t)p0 * 2);
    after_emit();
  });
}

}  // namespace

extern "C" {

int ppf_pca_portraits(ppf_ctx* ctx, int32_t nport, int32_t nchan, int32_t nbin, const double* port,
                      const double* weights, int32_t ncomp, double* mean_prof, double* eigval,
                      double* eigvec, int32_t* info) {
  if (!ctx || !port || !weights || !mean_prof || !eigval || !eigvec || !info)
    return fail(ctx, PPF_ERR_INVALID, "null argument");
  if (nport <= 0) return PPF_OK;
  int logN;
  if (int r = check_nbin_any(ctx, nbin, &logN)) return r;
  if (nchan < 2) return fail(ctx, PPF_ERR_INVALID, "nchan=%d: a PCA needs at least 2 rows", nchan);
  if (nchan > kPcaMaxRows)
    return fail(ctx, PPF_ERR_UNSUPPORTED, "nchan=%d: at most %d rows per portrait", nchan,
                kPcaMaxRows);
  if (ncomp < 1 || ncomp > std::min(nchan, nbin))
    return fail(ctx, PPF_ERR_INVALID, "ncomp=%d: 1..min(nchan, nbin)=%d", ncomp,
                std::min(nchan, nbin));
  HIPCHK(ctx, hipSetDevice(ctx->device));
  if (int r = pca_check_weights(ctx, weights, nport, nchan)) return r;
  // per portrait: A [nchan][nbin], |row|^2 [nchan], the state, the order [ncomp]
  const int m = nchan;
  WsPlan ws;
  const int wA = ws.array((size_t)m * nbin * sizeof(double));
  const int wN = ws.array((size_t)m * sizeof(double));
  const int wS = ws.array(sizeof(PcaState));
  const int wO = ws.array((size_t)ncomp * sizeof(int));
  // portraits per pass: under the workspace limit and the grid's y extent
  ws.lay_out(nport, ctx->ws_limit, 1024, 65535);
  if (int r = hold_workspace(ctx, ws)) return r;
  const PcaRows w{ws.at<double>(wA), ws.at<double>(wN), ws.at<PcaState>(wS), ws.at<int>(wO),
                  m, nbin, ncomp};
  for (int64_t p0 = 0; p0 < nport; p0 += ws.chunk) {
    const int np = (int)std::min<int64_t>(ws.chunk, nport - p0);
    if (int r = pca_reset(ctx, w, np)) return r;
    if (int r = timed(ctx, PPF_K_PCA, [&] {
          hipLaunchKernelGGL(k_pca_center, dim3((nbin + kBlock - 1) / kBlock, np), dim3(kBlock), 0,
                             ctx->stream, port + (size_t)p0 * m * nbin, weights + (size_t)p0 * m,
                             m, nbin, mean_prof + (size_t)p0 * nbin, w.A);
        }))
      return r;
    if (int r = pca_jacobi(ctx, w, np, [] {})) return r;
    if (int r = pca_emit(ctx, w, np, p0, eigval, eigvec, info, [] {})) return r;
  }
  return PPF_OK;
}

int ppf_pca_gram_portraits(ppf_ctx* ctx, int32_t nport, int32_t nchan, int32_t nbin,
                           const double* port, const double* weights, int32_t ncomp,
                           double* mean_prof, double* eigval, double* eigvec, int32_t* info) {
  if (!ctx || !port || !weights || !mean_prof || !eigval || !eigvec || !info)
    return fail(ctx, PPF_ERR_INVALID, "null argument");
  if (nport <= 0) return PPF_OK;
  int logN;
  if (int r = check_nbin_any(ctx, nbin, &logN)) return r;
  if (nbin > kPcaMaxRows)
    return fail(ctx, PPF_ERR_UNSUPPORTED, "nbin=%d: the covariance has at most %d rows", nbin,
                kPcaMaxRows);
  if (nchan < 2) return fail(ctx, PPF_ERR_INVALID, "nchan=%d: a PCA needs at least 2 rows", nchan);
  if (nchan > PPF_MAX_NCHAN)
    return fail(ctx, PPF_ERR_UNSUPPORTED, "nchan=%d: at most %d channels per portrait", nchan,
                PPF_MAX_NCHAN);
  if (ncomp < 1 || ncomp > std::min(nchan, nbin))
    return fail(ctx, PPF_ERR_INVALID, "ncomp=%d: 1..min(nchan, nbin)=%d", ncomp,
                std::min(nchan, nbin));
  HIPCHK(ctx, hipSetDevice(ctx->device));
  if (int r = pca_check_weights(ctx, weights, nport, nchan)) return r;
  // per portrait: G [nbin][nbin], the slabs' partial tiles, the row scales
  // [nchan], |row|^2 [nbin], trace(G), the state, the order [ncomp]
  const int m = nbin;
  const int npair = gram_npair(nbin), nslab = gram_nslab(nchan);
  WsPlan ws;
  const int wG = ws.array((size_t)m * nbin * sizeof(double));
  const int wP = ws.array((size_t)nslab * npair * kGramTile * kGramTile * sizeof(double));
  const int wC = ws.array((size_t)nchan * sizeof(double));
  const int wN = ws.array((size_t)m * sizeof(double));
  const int wT = ws.array(sizeof(double));
  const int wS = ws.array(sizeof(PcaState));
  const int wO = ws.array((size_t)ncomp * sizeof(int));
  // portraits per pass: under the workspace limit and the grid's z extent
  ws.lay_out(nport, ctx->ws_limit, 2048, 65535);
  if (int r = hold_workspace(ctx, ws)) return r;
  double* G = ws.at<double>(wG);
  double* part = ws.at<double>(wP);
  double* scale = ws.at<double>(wC);
  double* trace = ws.at<double>(wT);
  const PcaRows w{G, ws.at<double>(wN), ws.at<PcaState>(wS), ws.at<int>(wO), m, nbin, ncomp};
  // under timing, the device time of the launches since the last mark goes to phase i
  double seen = 0.0;
  auto mark = [&](int i) -> int {
    if (!ctx->timing) return PPF_OK;
    if (int r = resolve_timing(ctx)) return r;
    if (i >= 0) ctx->gram_ms[i] += ctx->ktime[PPF_K_PCA] - seen;
    seen = ctx->ktime[PPF_K_PCA];
    return PPF_OK;
  };
  if (int r = mark(-1)) return r;
  for (int64_t p0 = 0; p0 < nport; p0 += ws.chunk) {
    const int np = (int)std::min<int64_t>(ws.chunk, nport - p0);
    const double* x = port + (size_t)p0 * nchan * nbin;
    double* mean = mean_prof + (size_t)p0 * nbin;
    if (int r = pca_reset(ctx, w, np)) return r;
    if (int r = timed(ctx, PPF_K_PCA, [&] {
          hipLaunchKernelGGL(k_gram_mean, dim3((nbin + 63) / 64, np), dim3(64), 0, ctx->stream, x,
                             weights + (size_t)p0 * nchan, nchan, nbin, mean, scale);
        }))
      return r;
    if (int r = mark(0)) return r;
    if (int r = timed(ctx, PPF_K_PCA, [&] {
          hipLaunchKernelGGL(k_gram_tiles, dim3(gram_nsuper(nbin), nslab, np), dim3(kBlock), 0,
                             ctx->stream, x, scale, mean, nchan, nbin, npair, part);
        }))
      return r;
    if (int r = mark(1)) return r;
    if (int r = timed(ctx, PPF_K_PCA, [&] {
          hipLaunchKernelGGL(k_gram_reduce, dim3(npair, kGramTile / 4, np), dim3(kBlock), 0,
                             ctx->stream, part, nbin, nslab, G);
          hipLaunchKernelGGL(k_gram_trace, dim3(np), dim3(kBlock), 0, ctx->stream, G, nbin, trace);
        }))
      return r;
    if (int r = mark(2)) return r;
    // the Jacobi of ppf_pca_portraits on G's rows, with G's own null threshold
    if (int r = pca_jacobi(ctx, w, np, [&] {
          hipLaunchKernelGGL(k_gram_null, dim3((np + kBlock - 1) / kBlock), dim3(kBlock), 0,
                             ctx->stream, w.state, trace, nchan, np);
        }))
      return r;
    if (int r = mark(3)) return r;
    if (int r = pca_emit(ctx, w, np, p0, eigval, eigvec, info, [&] {
          hipLaunchKernelGGL(k_gram_sqrt, dim3((np * ncomp + kBlock - 1) / kBlock), dim3(kBlock),
                             0, ctx->stream, eigval + (size_t)p0 * ncomp, np * ncomp);
        }))
      return r;
    if (int r = mark(4)) return r;
  }
  return PPF_OK;
}

int ppf_pca_project(ppf_ctx* ctx, int32_t nport, int32_t nchan, int32_t nbin, const double* port,
                    const double* mean_prof, int32_t ncomp, const double* eigvec, double* proj,
                    double* reconst) {
  if (!ctx || !port || !mean_prof || !eigvec || !proj)
    return fail(ctx, PPF_ERR_INVALID, "null argument");
  if (nport <= 0) return PPF_OK;
  int logN;
  if (int r = check_nbin_any(ctx, nbin, &logN)) return r;
  if (nchan < 1) return fail(ctx, PPF_ERR_INVALID, "nchan=%d", nchan);
  if (nchan > PPF_MAX_NCHAN)
    return fail(ctx, PPF_ERR_UNSUPPORTED, "nchan=%d: at most %d channels per portrait", nchan,
                PPF_MAX_NCHAN);
  if (ncomp < 1 || ncomp > std::min<int>(kPcaMaxRows, nbin))
    return fail(ctx, PPF_ERR_INVALID, "ncomp=%d: 1..%d", ncomp, std::min<int>(kPcaMaxRows, nbin));
  HIPCHK(ctx, hipSetDevice(ctx->device));
  for (int64_t p0 = 0; p0 < nport; p0 += 65535) {  // the grid's y extent
    const int np = (int)std::min<int64_t>(65535, nport - p0);
    if (int r = timed(ctx, PPF_K_PCA, [&] {
          hipLaunchKernelGGL(k_pca_project, dim3(nchan, np), dim3(kBlock),
                             (size_t)ncomp * sizeof(double), ctx->stream,
                             port + (size_t)p0 * nchan * nbin, mean_prof + (size_t)p0 * nbin,
                             eigvec + (size_t)p0 * ncomp * nbin, nchan, nbin, ncomp,
                             proj + (size_t)p0 * nchan * ncomp,
                             reconst ? reconst + (size_t)p0 * nchan * nbin : nullptr);
        }))
      return r;
  }
  return PPF_OK;
}

}  // extern "C"
