/*
 * ppfit.h -- C ABI of libppfit.so, the MI355X (gfx950) implementation of the
 * PulsePortraiture wideband FFTFIT hot path.
 *
 * The reference (kmjc/PulsePortraiture) is pure Python; its "plugin surface"
 * is the set of Python call signatures listed in SURVEY.md §8(b).  Each entry
 * point below is what the Python drop-ins in pulseportraiture_amd/ bind via
 * ctypes in place of the reference's numpy/scipy code:
 *
 *   ppf_fit_portrait_batch  <- pptoaslib.fit_portrait_full   pptoaslib.py:928-1096
 *                              (+ the get_TOAs initial guess pptoas.py:420-456,
 *                               ppalign.py:180-185, batched over subints)
 *   ppf_fit_portrait_batch_raw <- the same on 16-bit PSRFITS samples: load_data's
 *                              scale / offset / pscrunch (pplib.py:2670-2732)
 *                              inside the fit's data pass
 *   ppf_phase_shift_batch   <- pplib.fit_phase_shift          pplib.py:2054-2100
 *   ppf_phase_tau_batch     <- pptoaslib.fit_portrait_full on one channel with
 *                              fit_flags [1,0,0,1,0]: the fit_phase_shift_scat
 *                              call that GetTOAs.get_narrowband_TOAs leaves
 *                              commented out (pptoas.py:752-753, 982-988;
 *                              objective pptoaslib.py:525-643, post-fit
 *                              pptoaslib.py:645-731)
 *   ppf_rotate_rows         <- pplib.rotate_data / rotate_portrait /
 *                              pptoaslib.rotate_portrait_full pplib.py:2338-2460,
 *                                                             pptoaslib.py:52-81
 *   ppf_rotate_accumulate   <- ppalign.align_archives' weighted sum
 *                              ppalign.py:202-208
 *   ppf_rotate_accumulate_spec <- the same sum over cached data spectra
 *                              (ppalign.py:202-208, iterations after the first)
 *   ppf_rotate_fscrunch     <- the dedispersed, weighted fscrunch per unit:
 *                              arch.fscrunch() in pplib.make_constant_portrait
 *                              (pplib.py:958-994) and the profiles psradd -P
 *                              aligns on (ppalign.py:21-38)
 *   ppf_scrunch_subints     <- arch.fscrunch() / bscrunch() of load_data
 *                              (pplib.py:2714) and pam -f / -b, from fp64
 *                              values or 16-bit samples (a stand-in, unpinned)
 *   ppf_irfft_rows          <- numpy.fft.irfft (final step of ppalign.py:210-213)
 *   ppf_noise_rows          <- pplib.get_noise_PS(chans=True)  pplib.py:2227-2253
 *   ppf_noise_fit_rows      <- pplib.get_noise_fit(chans=True) pplib.py:2255-2287
 *   ppf_find_kc_rows        <- pplib.find_kc                   pplib.py:1465-1495
 *   ppf_unpack_subints      <- PSRCHIVE Archive_load + pscrunch in
 *                              pplib.load_data  pplib.py:2670-2732 (with
 *                              include/ppfits.h, the host PSRFITS reader)
 *   ppf_profile_snr         <- Profile::snr() for load_data's SNRs
 *                              pplib.py:2762-2770 (PSRCHIVE restated)
 *   ppf_gaussian_portraits  <- pplib.gen_gaussian_portrait / read_model
 *                              pplib.py:853-930, 2873-2959
 *   ppf_scatter_rotate_rows <- GetTOAs.show_fit port/model  pptoas.py:1389-1402
 *   ppf_resid_chi2_rows     <- pplib.get_red_chi2 per channel in
 *                              GetTOAs.get_channels_to_zap  pptoas.py:1201-1278
 *   ppf_pca_portraits       <- pplib.pca                       pplib.py:1497-1534
 *   ppf_pca_gram_portraits  <- pplib.pca, more channels than bins (np.cov + eigh)
 *                              (as ppspline.make_spline_model calls it,
 *                              ppspline.py:67-82, batched over portraits)
 *   ppf_gauss_fit_batch     <- pplib.fit_gaussian_portrait     pplib.py:1924-2052
 *                              (lmfit's leastsq, batched over portraits;
 *                              ppf_gauss_eval is its objective)
 *   ppf_gauss_fit_join_batch <- the same with join_params (metafile portraits;
 *                              ppf_gauss_eval_join is its objective)
 *   ppf_powlaw_fit_rows     <- pplib.fit_powlaw                pplib.py:1763-1802
 *                              (lmfit's leastsq, batched over rows)
 *   ppf_line_fit_rows       <- np.polyfit in pplib.fit_DM_to_freq_resids
 *                              pplib.py:1804-1840
 *   ppf_gauss_bank          <- ppgauss.GaussianSelector (ppgauss.py:374-640,
 *                              a person at a plot): the matched-filter bank
 *                              of pplib.auto_gaussian_profiles
 *   ppf_pca_project         <- pplib.reconstruct_portrait and the projection
 *                              pplib.py:1536-1553, ppspline.py:119-129
 *   ppf_wavelet_smooth_rows <- pplib.wavelet_smooth            pplib.py:1621-1666
 *   ppf_wavelet_objective_rows <- pplib.fit_wavelet_smooth_function
 *                              pplib.py:1737-1761
 *   ppf_smart_smooth_rows   <- pplib.smart_smooth              pplib.py:1668-1735
 *                              (the db8 stationary transform from its
 *                              definition; PyWavelets in the reference)
 *   ppf_synth_portraits     <- (test/bench input producer; pplib.make_fake_pulsar
 *                              math, pplib.py:3342-3377, on device)
 *   ppf_fake_subints        <- pplib.make_fake_pulsar's data  pplib.py:3342-3379
 *                              (every polarisation, amplitude and noise level,
 *                              as 16-bit PSRFITS samples)
 *   ppf_pack_subints        <- PSRCHIVE's unload of amplitudes as 16-bit samples
 *                              in write_archive / unload_new_archive
 *                              pplib.py:3039-3187 (with include/ppfitsw.h, the
 *                              host PSRFITS writer)
 *
 * Conventions
 *  - Every array argument is a DEVICE pointer (hipMalloc'd or a torch CUDA
 *    tensor's data_ptr) unless documented otherwise; arrays are C-order fp64.
 *  - Calls are stream-ordered on the context's stream (ppf_set_stream); they
 *    do not synchronise unless stated.  One context per device per host
 *    thread; a context is not re-entrant.
 *  - Return codes: PPF_OK (0) or a negative PPF_ERR_*; ppf_last_error()
 *    describes the last failure.  Per-subint solver status follows scipy's
 *    trust-ncg codes (0 gradient small / NaN, 1 maxiter, 2 no predicted
 *    reduction, 3 linalg error), as returned by the reference's
 *    results.status (pptoaslib.py:1018).
 *  - Shapes (PPF_ERR_UNSUPPORTED with a message outside them, never a
 *    silent fallback): nbin in [16, 8192] and nchan <= PPF_MAX_NCHAN (the
 *    reference takes any; 16384 channels covers every receiver in use).
 *    The FFT kernels are built per power of two; for any other nbin (the
 *    reference's numpy rfft takes any length, pptoaslib.py:976-978)
 *    ppf_fit_portrait_batch, ppf_rotate_rows, ppf_scatter_rotate_rows,
 *    ppf_gaussian_portraits, ppf_spline_portraits,
 *    ppf_instrumental_response_rows, ppf_phase_shift_batch, ppf_phase_tau_batch,
 *    ppf_rotate_accumulate, ppf_rotate_fscrunch, ppf_irfft_rows, ppf_noise_rows and
 *    ppf_resid_chi2_rows run direct-sum kernels instead (O(nbin^2) per row;
 *    tests/test_gpu_generic_nbin.py), and so do the data-spectrum cache
 *    (PPF_SPEC_*, ppf_spec_nhp, ppf_rotate_accumulate_spec) and
 *    ppf_synth_portraits, ppf_fake_subints and ppf_pack_subints: every
 *    entry point takes any nbin in [16, 8192]
 *    (powers of two below 64 take the generic kernels too).  Of those
 *    lengths the even ones with nbin / 2 = 2^a 3^b 5^c take a mixed-radix
 *    FFT in the row entry points and the fit's data pass instead
 *    (ppf_row_transform, PPF_OPT_ROW_FFT).
 *  - Channel counts: up to PPF_LDS_NCHAN a fit workgroup keeps its subint's
 *    per-channel tables (frequencies, weights, dispersion derivatives, the
 *    fitted-channel list) in LDS; above it (or under PPF_OPT_HBM_TABLES) the
 *    same kernels, instantiated for it, keep them in an HBM workspace slice
 *    per workgroup, and scattering fits take one workgroup per subint
 *    (PPF_OPT_SCAT_SPLIT is not used).  The fits are bitwise the same either
 *    way (tests/test_gpu_wide.py); only their speed differs.
 */
#ifndef PPFIT_H
#define PPFIT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PPF_OK 0
#define PPF_ERR_INVALID -1
#define PPF_ERR_DEVICE -2
#define PPF_ERR_UNSUPPORTED -3
#define PPF_ERR_NOMEM -4

#define PPF_MAX_NCHAN 16384
#define PPF_LDS_NCHAN 2048
#define PPF_VERSION 1

/* kernel ids for ppf_get_kernel_time */
#define PPF_K_MODEL_FFT 0
#define PPF_K_DATA_XSPEC 1
#define PPF_K_SOLVE 2
#define PPF_K_PHASE_SHIFT 3
#define PPF_K_ROTATE 4
#define PPF_K_ROT_ACCUM 5
#define PPF_K_SYNTH 6
#define PPF_K_IRFFT 7
#define PPF_K_NOISE 8
#define PPF_K_GUESS 9
#define PPF_K_POST 10
#define PPF_K_FIT_TAYLOR 11
#define PPF_K_MOMENTS 12
#define PPF_K_RESID 13
#define PPF_K_UNPACK 14
#define PPF_K_PCA 15
#define PPF_K_GAUSS 16
#define PPF_K_PACK 17
#define PPF_K_SWT 18
#define PPF_K_GBANK 19
#define PPF_K_FSCRUNCH 20
#define PPF_NUM_KERNELS 21

typedef struct ppf_ctx ppf_ctx;

int ppf_version(void);
int ppf_ctx_create(int device, ppf_ctx** out);
void ppf_ctx_destroy(ppf_ctx* ctx);
const char* ppf_last_error(const ppf_ctx* ctx);
/* hip stream (hipStream_t cast to void*); NULL selects the null stream */
int ppf_set_stream(ppf_ctx* ctx, void* stream);
int ppf_synchronize(ppf_ctx* ctx);
/* Phase-family fits (trust-ncg, no tau/alpha) split each workspace chunk
 * into `pieces` launches alternating between the context stream and a
 * second internal queue, piece p's data pass ordered after piece p-1's, so
 * one piece's latency-bound solver kernels overlap the next one's HBM-bound
 * pass.  Results are bitwise those of pieces = 1.  0 = the library default
 * (1: measured no faster); at most 64.                        */
int ppf_set_pipeline(ppf_ctx* ctx, int32_t pieces);
/* Launch-schedule options of one context (diagnostic / A-B use; the
 * library reads no environment variables).  None of them changes a
 * result: every setting gives bitwise the same fits (tests/test_gpu_options.py).
 *   PPF_OPT_SCAT_GRAPH   1: the split scattering solve launches each group of
 *                        four iterations as one hipGraph (default); 0: one
 *                        launch per kernel.
 *   PPF_OPT_SCAT_SPLIT   1: trust-ncg scattering fits spread every evaluation
 *                        over several workgroups (k_scat_sweep/k_scat_step,
 *                        default); 0: one workgroup per subint (k_solve).
 *   PPF_OPT_SCAT_TAIL    running subints below which the split solve takes
 *                        one 8-channel group per wave (default 512; 0 never).
 *   PPF_OPT_FUSE_MOMENTS 1: the first Taylor moment pass runs inside
 *                        k_fit_taylor (default); 0: its own k_moments launch.
 *   PPF_OPT_GUESS_WAVE   1: the single-wave guess kernel takes the subints it
 *                        covers (default); 0: every guess in k_guess.
 *   PPF_OPT_HBM_TABLES   1: the per-channel tables in HBM at every channel
 *                        count (default 0: only above PPF_LDS_NCHAN).
 *   PPF_OPT_POST_WAVE    1: the single-wave post-fit kernel (k_post_w) takes
 *                        the phase-family fits it covers (default); 0: every
 *                        post-fit in k_post.
 * One option chooses between two implementations of the same transform, so
 * its two settings agree to rounding (1e-12 of a row's scale), not bitwise:
 *   PPF_OPT_ROW_FFT      1: an even nbin with nbin / 2 = 2^a 3^b 5^c that is
 *                        no power of two from 64 up takes the mixed-radix row
 *                        FFT (default; ppf_row_transform answers
 *                        PPF_ROW_SMOOTH); 0: every such length takes the
 *                        direct sums and the fit's data pass the DFT on the
 *                        matrix cores, as every other non-power-of-two length
 *                        does.  Powers of two from 64 up are bitwise the same
 *                        under either value.                                */
#define PPF_OPT_SCAT_GRAPH 0
#define PPF_OPT_SCAT_SPLIT 1
#define PPF_OPT_SCAT_TAIL 2
#define PPF_OPT_FUSE_MOMENTS 3
#define PPF_OPT_GUESS_WAVE 4
#define PPF_OPT_HBM_TABLES 5
#define PPF_OPT_POST_WAVE 6
#define PPF_OPT_ROW_FFT 7
#define PPF_NUM_OPTS 8
int ppf_set_option(ppf_ctx* ctx, int32_t option, int32_t value);
int ppf_get_option(const ppf_ctx* ctx, int32_t option, int32_t* value);
/* Upper bound on workspace bytes the context may hold (default 32 GiB). */
int ppf_set_workspace_limit(ppf_ctx* ctx, int64_t bytes);
int ppf_get_workspace_limit(const ppf_ctx* ctx, int64_t* bytes);
/* Per-kernel HIP-event timing on the context stream (off by default). */
int ppf_set_timing(ppf_ctx* ctx, int enable);
/* Diagnostic: record every objective sweep of the TNC and Newton-CG solvers
 * and of the split trust-ncg scattering solve (the point, f, gradient,
 * Hessian terms, whether it counts in nfev) into buf [nsub][cap][32]
 * doubles (device memory, caller-owned; batch subint index), at most cap
 * sweeps per subint.  cap 0 turns it off.  Split scattering records also
 * hold, in fields 28-31, the trust radius after the evaluation's update,
 * the predicted reduction and rho of the step that led to it, and its
 * Steihaug boundary flag.                                                 */
int ppf_set_trace(ppf_ctx* ctx, double* buf, int32_t cap);
int ppf_get_kernel_time(ppf_ctx* ctx, int kernel_id, double* total_ms,
                        int64_t* launches);
int ppf_reset_kernel_times(ppf_ctx* ctx);
/* ms[5]: the PPF_K_PCA time of ppf_pca_gram_portraits calls made under
 * ppf_set_timing since the last reset, split into the mean pass, the Gram
 * tiles, the sum over slabs (with the trace), the Jacobi on G and the emit. */
int ppf_get_pca_gram_times(ppf_ctx* ctx, double* ms);
/* Device self-test of the cross-lane primitives the kernels rely on
 * (DPP row/quad moves, permlane16/32 swaps, readlane).  fails[t] (t <
 * PPF_SELFTEST_N) = number of lanes where test t is wrong; all 0 = pass.   */
#define PPF_SELFTEST_N 10
int ppf_selftest(ppf_ctx* ctx, int32_t* fails);
/* Diagnostic phase clock of the Taylor fit kernel (off by default).  When
 * enabled, every k_fit_taylor workgroup adds its wall_clock64 ticks (100 MHz)
 * per phase into device counters: out[0] guess, [1] meta + first moments,
 * [2] centre selection incl. recentring, [3] objective sweeps, [4] trust-
 * region step, [8] recentring passes, [9] workgroups; every k_post or
 * k_post_w workgroup likewise: [16] meta + Sd, [17] nu_zero sums and solve, [18]
 * outputs at nu_out + centre pick, [19] with-scales sweep, [20] inverses,
 * [21] per-channel errors + stores, [22] workgroups.  The call copies the
 * counters to out (if non-null), zeroes them and sets the enable state.   */
#define PPF_PHASE_N 32
int ppf_phase_profile(ppf_ctx* ctx, int32_t enable, uint64_t* out);

/* ---------------------------------------------------------------------- */
/* Batched wideband fit: fit_portrait_full over nsub subints.              */
/* ---------------------------------------------------------------------- */
/* minimize() method of fit_portrait_full (pptoaslib.py:995-1014)          */
#define PPF_METHOD_TRUST_NCG 0   /* scipy trust-ncg, gtol = -1 (the default)  */
#define PPF_METHOD_TNC 1         /* scipy TNC with bounds, xtol 1e-10, minfev */
#define PPF_METHOD_NEWTON_CG 2   /* scipy Newton-CG, xtol = -1, maxiter 2000   */
#define PPF_METHOD_TNC_LEGACY 3  /* pplib.fit_portrait: TNC over (phase, DM) only,
                                    xtol 1e-10 (pplib.py:2144-2148); fit_flags
                                    must be [1,1,0,0,0]                        */

/* Phase-family fits (tau = 0 and not fitted) evaluate the objective from
 * per-channel Taylor moments of the cross-spectrum (no nchan x nharm
 * workspace).  PPF_SOLVE_EXACT forces the exact cross-spectrum sweeps
 * instead (same results to rounding; used to cross-check the two).
 * PPF_SOLVE_EVAL evaluates f, g, H and the post-fit at init without any
 * solver step (status 1, nfev 1): the objective-kernel parity hook for
 * fit_portrait_full_function{,_deriv,_2deriv} (pptoaslib.py:525-643).
 * PPF_GUESS_DIRECT takes the brute-force grid of the initial guess by
 * direct sums instead of the folded L-point DFT.                          */
#define PPF_SOLVE_EXACT 1
#define PPF_SOLVE_EVAL 2
#define PPF_GUESS_DIRECT 4

/* Data-spectrum cache (spec_mode; ppalign's iterations, ppalign.py:160-213,
 * refit the same subints against each new template).  The cache is the
 * caller's: spec [nsub][nchan][NHP] complex (interleaved re, im; NHP =
 * ppf_spec_nhp(nbin)), spec_sig and spec_dsum [nsub][nchan], spec_R
 * [nsub][NHP] complex.
 *   PPF_SPEC_STORE: the data pass also stores each subint's spectrum (rfft
 *     of the row, DC included), noise sigma, sum |D|^2 / sigma^2 and guess
 *     average in the cache (every other output as without the cache);
 *   PPF_SPEC_USE: no data pass -- those come from the cache, and the Taylor
 *     moment passes form the cross-spectrum D conj(M) from the cached
 *     spectrum as they stream it: the same X, bitwise, so the same fits.
 *     Only phase-family trust-ncg fits (tau = 0, not fitted; not
 *     PPF_SOLVE_EXACT) take it, with the data, freqs, errs, mask, weights, P
 *     and guess_nu of the STORE call.                                    */
#define PPF_SPEC_NONE 0
#define PPF_SPEC_STORE 1
#define PPF_SPEC_USE 2
int32_t ppf_spec_nhp(int32_t nbin);

/* Which row transform the entry points launch for nbin under ctx's options
 * (ctx NULL: the default options); no device needed.  *kind:
 *   PPF_ROW_POW2    a power of two from 64 up: the LDS and register FFTs;
 *   PPF_ROW_SMOOTH  an even nbin with nbin / 2 = 2^a 3^b 5^c (96, 100, 768,
 *                   1000, 1536, 2000, 3000, 6144, 8000, ...; 16 and 32 too):
 *                   the mixed-radix LDS FFT, O(nbin log nbin) per row, in the
 *                   row entry points and the fit's data pass
 *                   (PPF_OPT_ROW_FFT 0: PPF_ROW_DIRECT instead);
 *   PPF_ROW_DIRECT  every other length (odd, or a prime factor above 5 in
 *                   nbin / 2, such as 8190): direct sums, O(nbin^2) per row.
 * The wavelet, noise-fit-grid, Gaussian and narrowband-tau kernels use their
 * direct sums for PPF_ROW_SMOOTH lengths as for PPF_ROW_DIRECT ones.
 * Returns PPF_ERR_UNSUPPORTED outside [16, 8192].                           */
#define PPF_ROW_POW2 0
#define PPF_ROW_SMOOTH 1
#define PPF_ROW_DIRECT 2
int ppf_row_transform(const ppf_ctx* ctx, int32_t nbin, int32_t* kind);

typedef struct {
  int32_t nsub, nchan, nbin, nmodel;
  int32_t fit_flags[5];   /* phi, DM, GM, tau, alpha (pptoaslib.py:928)     */
  int32_t log10_tau;      /* fit log10(tau) instead of tau                 */
  int32_t option;         /* get_nu_zeros option (pptoaslib.py:733)        */
  int32_t method;         /* PPF_METHOD_*                                   */
  int32_t is_toa;         /* pptoaslib.py:1048-1050                         */
  int32_t guess;          /* 1: in-kernel initial phase guess (pptoas.py:420-456) */
  int32_t guess_Ns;       /* opt.brute grid size (100 in pptoas, nbin in ppalign) */
  int32_t guess_wrap;     /* 1: phase_transform(..., mod=True) to nu_fit_DM */
  int32_t solver_flags;   /* PPF_SOLVE_* bits (0 = default)                */
  const double* data;       /* [nsub][nchan][nbin]                          */
  const double* model;      /* [nmodel][nchan][nbin]                        */
  const int32_t* model_idx; /* [nsub] or NULL (all 0)                       */
  const double* freqs;      /* [nsub][nchan] MHz                            */
  const double* errs;       /* [nsub][nchan] time-domain sigma; NULL or a NaN
                               entry: estimated as get_noise_PS (pplib.py:2227) */
  const uint8_t* chan_mask; /* [nsub][nchan] 1 = fit channel, or NULL       */
  const double* weights;    /* [nsub][nchan] guess-average weights or NULL  */
  const double* P;          /* [nsub] period, s                             */
  const double* init;       /* [nsub][5] initial params                     */
  const double* nu_fit;     /* [nsub][3] NaN -> mean of fitted freqs        */
  const double* nu_out;     /* [nsub][3] NaN -> zero-covariance frequency   */
  const double* guess_nu;   /* [nsub] dedispersion ref of the guess; NaN ->
                               mean freq (pptoas) ; NULL -> NaN             */
  const double* guess_tau;  /* [nsub] linear tau [rot] at nu_fit_tau applied
                               to the guess template, or NULL (0)           */
  const double* bounds;     /* HOST pointer, [5][2] (low, high) per parameter
                               for the whole batch, NaN = None; read by
                               PPF_METHOD_TNC only (NULL = all None)        */
  int32_t spec_mode;        /* PPF_SPEC_* (data-spectrum cache, above)       */
  double* spec;             /* [nsub][nchan][NHP] complex, or NULL            */
  double* spec_sig;         /* [nsub][nchan]                                  */
  double* spec_dsum;        /* [nsub][nchan]                                  */
  double* spec_R;           /* [nsub][NHP] complex                            */
} ppf_fit_desc;

typedef struct {
  double* params;       /* [nsub][5] (phi at nu_DM, DM, GM, tau(log10?), alpha) */
  double* param_errs;   /* [nsub][5]                                        */
  double* nu_out;       /* [nsub][3] nu_DM, nu_GM, nu_tau                  */
  double* cov;          /* [nsub][5][5] nfit x nfit block top-left           */
  double* scales;       /* [nsub][nchan] (0 on masked channels)             */
  double* scale_errs;   /* [nsub][nchan]                                    */
  double* channel_snrs; /* [nsub][nchan]                                    */
  double* chi2;         /* [nsub]                                           */
  double* red_chi2;     /* [nsub]                                           */
  double* snr;          /* [nsub]                                           */
  int32_t* nfev;        /* [nsub]                                           */
  int32_t* status;      /* [nsub]                                           */
  double* init_used;    /* [nsub][5] or NULL: starting point after the guess */
  double* fun;          /* [nsub] or NULL: final objective value            */
  double* cov_nosc;     /* [nsub][5][5] or NULL: inv(0.5 H) of the curvature
                           without amplitude terms at the output params
                           (legacy pplib.fit_portrait errors, pplib.py:2184-2190) */
  double* grad;         /* [nsub][5] or NULL: gradient at the final point (jac) */
  double* hess;         /* [nsub][5][5] or NULL: Hessian at the final point     */
  double* errs_out;     /* [nsub][nchan] or NULL: the time-domain noise sigma
                           each channel was fitted with -- desc->errs, or
                           get_noise_PS of the row where that is NULL / NaN
                           (pplib.py:2227-2253); 0 for masked channels.  Lets
                           a caller weight by load_data's noise_stds without
                           a separate noise pass (ppalign.py:202-208)      */
} ppf_fit_result;

int ppf_fit_portrait_batch(ppf_ctx* ctx, const ppf_fit_desc* desc,
                           const ppf_fit_result* out);

/* The same fit straight from PSRFITS samples: the data pass reads the 16-bit
 * samples and forms value = raw * scl + offs (the polarisation sum of pmode
 * 1 included) as it loads each row, so no fp64 copy of the data exists.
 * Every output is bit for bit that of ppf_unpack_subints followed by
 * ppf_fit_portrait_batch.  desc is ppf_fit_desc unchanged, with desc->data
 * NULL (else PPF_ERR_INVALID); everything else of the call -- methods, flags,
 * masks, the data-spectrum cache, the chunk loop -- is as there.
 * PPF_ERR_UNSUPPORTED unless raw_type is PPFITS_RAW_I16 and nbin is a power
 * of two in [64, 8192] (unpack and call ppf_fit_portrait_batch for those);
 * PPF_ERR_INVALID for pmode outside 0..2, ipol >= npol, pmode 1 with npol < 2
 * or raw not 16-byte aligned.                                              */
typedef struct {
  int32_t raw_type;   /* PPFITS_RAW_* of ppfits.h; PPFITS_RAW_I16 here        */
  int32_t npol;       /* polarisations stored per subint                      */
  int32_t pmode;      /* as ppf_unpack_subints: 0 one polarisation (ipol),
                         1 AA + BB (p = 0 and 1), 2 the first (Stokes I)      */
  int32_t ipol;       /* pmode 0: which polarisation is fitted                */
  const void*   raw;  /* [nsub][npol][nchan][nbin]                            */
  const double* scl;  /* [nsub][npol][nchan]                                  */
  const double* offs; /* [nsub][npol][nchan]                                  */
} ppf_raw_subints;

int ppf_fit_portrait_batch_raw(ppf_ctx* ctx, const ppf_fit_desc* desc,
                               const ppf_raw_subints* raw, const ppf_fit_result* out);

/* ---------------------------------------------------------------------- */
/* fit_phase_shift over nprof profiles (pplib.py:2054-2100).              */
/* out[nprof][6] = phase, phase_err, scale, scale_err, snr, red_chi2       */
/* noise: [nprof] time-domain sigma or NaN/NULL -> get_noise (PS)          */
/* ---------------------------------------------------------------------- */
int ppf_phase_shift_batch(ppf_ctx* ctx, int32_t nprof, int32_t nbin,
                          const double* data, const double* model,
                          const int32_t* model_idx, const double* noise,
                          int32_t Ns, double lo, double hi, double* out);

/* ---------------------------------------------------------------------- */
/* A phase and a scattering time per profile: fit_portrait_full             */
/* (pptoaslib.py:928-1096) on each row as a one-channel portrait with       */
/* fit_flags [1, 0, 0, 1, 0] and nu_fits = nu_outs = the channel's own      */
/* frequency, by scipy's trust-ncg (gtol -1, maxiter 1000); one wave per    */
/* profile (ppfit_nbscat.hip).  16 <= nbin <= 8192 (PPF_ERR_UNSUPPORTED     */
/* otherwise).                                                              */
/*   model[nmodel][nbin]: the unscattered template rows; model_idx[nprof]   */
/*     (int32, or NULL: row 0) picks each profile's.                        */
/*   noise[nprof]: time-domain sigma, or NaN / NULL -> get_noise_PS of the  */
/*     row (pplib.py:2227-2253).                                            */
/*   tau0[nprof] (or NULL): starting tau in rotations, linear; <= 0 or NaN  */
/*     starts at 1 / nbin.  The starting phase is the peak of the           */
/*     cross-correlation with the template scattered at the starting tau,   */
/*     on min(nbin, 256) phases.                                            */
/*   log10_tau != 0: the fitted parameter t is log10(tau), else tau.        */
/*   out[nprof][9] = phi, phi_err, t, t_err, scale, scale_err, snr,         */
/*     red_chi2 (dof nbin - 3), cov(phi, t).                                */
/*   status[nprof], nfev[nprof] (int32): scipy's status code and its count  */
/*     of objective evaluations.                                            */
/* A profile's results do not depend on what shares the call.               */
/* ---------------------------------------------------------------------- */
int ppf_phase_tau_batch(ppf_ctx* ctx, int32_t nprof, int32_t nbin,
                        const double* data, const double* model,
                        const int32_t* model_idx, const double* noise,
                        const double* tau0, int32_t log10_tau, double* out,
                        int32_t* status, int32_t* nfev);

/* Principal components of nport portraits (pplib.pca, pplib.py:1497-1534):
 * mean_prof[p] = sum_n w[p][n] port[p][n] / sum_n w[p][n] (channels in
 * order), and the ncomp leading eigenvalues (descending) and unit
 * eigenvectors of np.cov((port[p] - mean_prof[p]).T, aweights=w[p], ddof=1).
 * They are the squared singular values and right singular vectors of
 * A[n] = sqrt(w_n / fact) (port[n] - mean), fact = sum w - sum w^2 / sum w,
 * from a one-sided Jacobi on A's rows in fp64 (ppfit_pca.hip): no nbin x
 * nbin matrix is formed, and of the reference's nbin eigenvectors at most
 * min(nchan, nbin) exist here (the rest span the null space).  Rows whose
 * |row|^2 is at most eps^2 nbin times the largest are null and left as they
 * are: the vectors of eigenvalues that small (rank-deficient input: at most
 * nchan - 1 are non-zero) are unit vectors of no meaning, or zeros.
 *   Sign: each vector's largest-magnitude component, the first on ties, is
 * positive (LAPACK's is arbitrary).  Results are bitwise reproducible and do
 * not depend on how many portraits share the call.
 *   2 <= nchan <= 2048 rows, 1 <= ncomp <= min(nchan, nbin).  Weights are
 * finite and >= 0 with at least two > 0 per portrait (PPF_ERR_INVALID
 * otherwise: fact would be 0); a zero-weight row contributes nothing.
 *   info[p] = {sweeps made, 1 if converged (a sweep without a rotation)
 * within 30 sweeps else 0}.  The copy of A is workspace
 * (ppf_set_workspace_limit splits the call over portraits).  The call
 * synchronises the stream once per sweep.                                  */
int ppf_pca_portraits(ppf_ctx* ctx, int32_t nport, int32_t nchan, int32_t nbin,
                      const double* port /* [nport][nchan][nbin] */,
                      const double* weights /* [nport][nchan] */, int32_t ncomp,
                      double* mean_prof /* [nport][nbin] */, double* eigval /* [nport][ncomp] */,
                      double* eigvec /* [nport][ncomp][nbin]: vectors as rows */,
                      int32_t* info /* [nport][2] */);

/* The same principal components from the nbin x nbin covariance itself, as
 * the reference forms it (np.cov, then eigh): for portraits with more
 * channels than bins, where the rows of A outnumber its rank.  G = A^T A is
 * summed on the fp64 matrix cores (ppfit_gram.hip) without storing A: 64 x
 * 64 tiles of the lower triangle, the channels in slabs of 256 whose partial
 * tiles meet in a second launch in slab order, the upper triangle a copy.
 * The Jacobi of ppf_pca_portraits then runs on G's nbin rows; the norms of
 * the rotated rows are the eigenvalues.  Rows of norm at most
 * nchan eps trace(G), the bound on |G - exact|_F, are null beside the rows
 * entry's own floor.  mean_prof is bitwise ppf_pca_portraits'; eigenvalues
 * and vectors agree with it to rounding, not bitwise.  Sign, order, info,
 * the weights' rules and the reproducibility contract are the sister
 * entry's.
 *   2 <= nchan <= PPF_MAX_NCHAN, 16 <= nbin <= 2048 (PPF_ERR_UNSUPPORTED
 * above either limit), 1 <= ncomp <= min(nchan, nbin).  G and the partial
 * tiles are workspace (ppf_set_workspace_limit splits the call over
 * portraits).                                                              */
int ppf_pca_gram_portraits(ppf_ctx* ctx, int32_t nport, int32_t nchan, int32_t nbin,
                           const double* port /* [nport][nchan][nbin] */,
                           const double* weights /* [nport][nchan] */, int32_t ncomp,
                           double* mean_prof /* [nport][nbin] */,
                           double* eigval /* [nport][ncomp] */,
                           double* eigvec /* [nport][ncomp][nbin]: vectors as rows */,
                           int32_t* info /* [nport][2] */);

/* proj[p][n][e] = (port[p][n] - mean_prof[p]) . eigvec[p][e] and, when
 * reconst is not NULL, reconst[p][n] = sum_e proj[p][n][e] eigvec[p][e] +
 * mean_prof[p] (reconstruct_portrait, pplib.py:1536-1553).  nchan <=
 * PPF_MAX_NCHAN, 1 <= ncomp <= min(2048, nbin); proj [nport][nchan][ncomp], reconst
 * [nport][nchan][nbin].                                                    */
int ppf_pca_project(ppf_ctx* ctx, int32_t nport, int32_t nchan, int32_t nbin, const double* port,
                    const double* mean_prof, int32_t ncomp, const double* eigvec, double* proj,
                    double* reconst);

/* Wavelet smoothing of profiles (pplib.wavelet_smooth, pplib.py:1621-1666):
 * the undecimated db8 transform with periodic extension to nlevel[r] levels,
 * the threshold lambda = fact[r] median(|a_L u d_L|) / 0.6745 sqrt(2 ln nbin)
 * applied to a_L and every d_j (PPF_THRESH_HARD: c -> 0 where |c| < lambda;
 * PPF_THRESH_SOFT: c -> sign(c) max(|c| - lambda, 0)), and the linear inverse
 * (DESIGN.md section 9 has the definition; it is built from that definition
 * and is not pinned against PyWavelets).  nbin even in [16, 8192]
 * (PPF_ERR_UNSUPPORTED otherwise); every nlevel[r] in 1 .. 13 with nbin a
 * multiple of 2^nlevel (PPF_ERR_INVALID otherwise; the levels are read on
 * the host, one stream synchronisation).  The coefficients are workspace
 * (ppf_set_workspace_limit splits the call over rows).  Results are bitwise
 * reproducible and a row's do not depend on the other rows of the call.    */
#define PPF_THRESH_HARD 0
#define PPF_THRESH_SOFT 1
int ppf_wavelet_smooth_rows(ppf_ctx* ctx, int32_t nrow, int32_t nbin,
                            const double* rows /* [nrow][nbin] */,
                            const int32_t* nlevel /* [nrow] */, const double* fact /* [nrow] */,
                            int32_t threshtype, double* out /* [nrow][nbin] */);

/* pplib.fit_wavelet_smooth_function (pplib.py:1737-1761) of each row at its
 * (nlevel, fact): obj[r] = -sum_{k>=1} |rfft(s)_k|^2 / (get_noise_PS(s)
 * sqrt(nbin / 2)) for the smoothed row s -- 0 when the signal is 0, -inf
 * when the noise is 0, 0 when |red_chi2 - 1| > rchi2_tol -- and red_chi2[r] =
 * sum ((row - s) / get_noise_PS(row))^2 / nbin (get_red_chi2).             */
int ppf_wavelet_objective_rows(ppf_ctx* ctx, int32_t nrow, int32_t nbin, const double* rows,
                               const int32_t* nlevel, const double* fact, int32_t threshtype,
                               double rchi2_tol, double* obj /* [nrow] */,
                               double* red_chi2 /* [nrow] */);

/* pplib.smart_smooth (pplib.py:1668-1735) of each row: for every level 1 ..
 * try_nlevels, scipy.optimize.brute of the objective above over fact on
 * linspace(0, 3, 30) (the first minimum) and its fmin finish from that point;
 * then the first level of least objective, the row smoothed there, and zeros
 * instead when its red_chi2 is further than rchi2_tol from 1 (zeroed[r] = 1).
 * An all-zero row stays zero (nlevel 0).  nbin a multiple of 2^try_nlevels,
 * 1 <= try_nlevels <= 13.  table, when not NULL, receives the polished
 * objective of every (row, level), [nrow][try_nlevels].                    */
int ppf_smart_smooth_rows(ppf_ctx* ctx, int32_t nrow, int32_t nbin, const double* rows,
                          int32_t try_nlevels, double rchi2_tol, int32_t threshtype,
                          double* out /* [nrow][nbin] */, int32_t* nlevel /* [nrow] */,
                          double* fact /* [nrow] */, double* red_chi2 /* [nrow] */,
                          int32_t* zeroed /* [nrow] */, double* table);

/* out[r] = irfft(rfft(in[r]) * exp(2 pi i k phase[r]))  (rotate_data)     */
int ppf_rotate_rows(ppf_ctx* ctx, int32_t nrow, int32_t nbin, const double* in,
                    const double* phase, double* out);

/* accum[n][k] += sum_s weight[s][n] * rfft(data[s][n])[k] * e^{2 pi i k phase[s][n]}
 * accum is complex [nchan][nbin/2+1] interleaved (re, im); weight 0 skips.  */
int ppf_rotate_accumulate(ppf_ctx* ctx, int32_t nsub, int32_t nchan,
                          int32_t nbin, const double* data, const double* phase,
                          const double* weight, double* accum);
/* The same sum from cached spectra (PPF_SPEC_STORE's spec, [nsub][nchan][NHP]
 * complex): no FFT, one pass over the spectra.  Rows of channels the fit
 * masked hold zeros (give them weight 0, as ppalign does).               */
int ppf_rotate_accumulate_spec(ppf_ctx* ctx, int32_t nsub, int32_t nchan,
                               int32_t nbin, const double* spec, const double* phase,
                               const double* weight, double* accum);

/* Rotate and frequency-scrunch: for every unit u (an archive or a subint)
 *   prof[u] = irfft(sum_n weight[u][n] rfft(data[u][n]) e^{2 pi i k phase[u][n]}, n = nbin)
 * i.e. sum_n weight[u][n] * ppf_rotate_rows(data[u][n], phase[u][n]); data
 * [nunit][nchan][nbin], phase and weight [nunit][nchan], prof [nunit][nbin].
 * Channels of weight 0 are skipped; nchan <= 0 gives zeros.  The channels are
 * summed in a fixed order that does not depend on nunit (slices of a fixed
 * number of channels, then the slices in order, no atomics): a unit's profile
 * is bitwise the same alone or among other units, and from run to run.      */
int ppf_rotate_fscrunch(ppf_ctx* ctx, int32_t nunit, int32_t nchan, int32_t nbin,
                        const double* data, const double* phase, const double* weight,
                        double* prof);

/* Frequency- and bin-scrunch subints: the stand-in for `pam -f / -b`, NOT
 * pinned against pam.  For every subint s, kept polarisation p and group g of
 * f adjacent channels (n in g: channels g f .. g f + f - 1),
 *   W            = sum_{n in g} w[s][n]
 *   y            = irfft(sum_{n in g, w != 0} w[s][n] rfft(x[s][p][n])_k e^{2 pi i k phase[s][n]},
 *                        nbin) / W
 *   out[s][p][g][j] = (1/b) sum_{i < b} y[j b + i]        wout[s][g] = W
 * A group with W = 0 gives zeros and weight 0; a sample under weight 0 never
 * enters a sum (a NaN there is harmless).  weights and phase [nsub][nchan],
 * out [nsub][npol][nchan/f][nbin/b], wout [nsub][nchan/f]; device pointers.
 * Exactly one of data and raw is given:
 *   data  fp64 [nsub][npol][nchan][nbin] -- viewed as [nsub npol nchan/f][f][nbin]
 *         it is what ppf_rotate_fscrunch sums, by the same kernels;
 *   raw   16-bit PSRFITS samples (ppf_raw_subints above), read as they are:
 *         no fp64 copy of the data exists, and every output is bit for bit
 *         that of ppf_unpack_subints followed by this call on its values.
 *         pmode 1 and 2 keep one polarisation (npol = 1); pmode 0 keeps
 *         polarisation ipol (npol = 1) or, with ipol < 0, every stored one
 *         (npol = raw->npol).  PPF_ERR_UNSUPPORTED unless raw_type is
 *         PPFITS_RAW_I16 and nbin a power of two in [64, 8192]: unpack those
 *         first, in bounded chunks (Engine.scrunch_subints does).
 * The bins are averaged as they stand, with no compensating rotation: bin j
 * of the output is centred (b - 1) / (2 nbin) of a turn later than bin j b
 * of the input.  PPF_ERR_INVALID: a null pointer, f not dividing nchan, b
 * not dividing nbin; PPF_ERR_UNSUPPORTED: nbin / b < 16, nbin outside
 * [16, 8192].  A group's output is bitwise the same whatever else shares the
 * call and under any workspace limit (the channel order of
 * ppf_rotate_fscrunch; units are chunked, never split).                     */
int ppf_scrunch_subints(ppf_ctx* ctx, int32_t nsub, int32_t npol, int32_t nchan, int32_t nbin,
                        const double* data, const ppf_raw_subints* raw, const double* weights,
                        const double* phase, int32_t f, int32_t b, double* out, double* wout);

/* Gaussian-component template rows (gen_gaussian_portrait, pplib.py:853-930,
 * as read_model calls it, pplib.py:2873-2959): out[r][:] at freqs[r] for
 * nrow rows (portraits x channels, any mix of frequencies).  code: HOST
 * int32[3], the evolution of loc / wid / amp (0 power law, 1 linear:
 * evolve_parameter, pplib.py:1030-1046); params: HOST double[2 + 6 ngauss],
 * DC, TAU [bin] (read_model's TAU * nbin / P), then per component loc,
 * dloc, wid, dwid, amp, damp; ngauss <= 32.  TAU != 0 scatters row r by
 * TAU / nbin (freqs[r] / nu_ref)^alpha.  out may not alias freqs.        */
int ppf_gaussian_portraits(ppf_ctx* ctx, int32_t nrow, int32_t nbin, int32_t ngauss,
                           const int32_t* code, const double* params, double nu_ref,
                           double alpha, const double* freqs, double* out);

/* Gaussian-component portrait fits (fit_gaussian_portrait, pplib.py:1924-2052;
 * ppfit_gauss.hip).  nport portraits of one shape [nchan][nbin]; everything
 * below is DEVICE memory.  The external parameter vector of a portrait has
 * npar = 3 + 6 ngauss entries: DC, tau [bin], per component loc, dloc, wid,
 * dwid, amp, damp, and last the scattering index alpha.  The residual is
 * (data - gen_gaussian_portrait(code, params[:-1], alpha, ..., freqs, nu_ref))
 * / errs (pplib.py:1230-1242) with the portrait as ppf_gaussian_portraits
 * builds it; errs are constant along a row ([nport][nchan], > 0).  The
 * Jacobian is analytic (the rescale factor, the wrap and the |z| < 20
 * support held fixed).
 *   Limits: ngauss <= 16, nchan <= 2048, nbin a power of two in [64, 8192]
 * (PPF_ERR_UNSUPPORTED otherwise).  Scratch is workspace
 * (ppf_set_workspace_limit splits the call over portraits).  Results are
 * bitwise reproducible and do not depend on how many portraits share the
 * call.
 *
 * ppf_gauss_eval: at params [nport][npar], chi2[p] = |r|^2, jtr [nport][npar]
 * = J^T r and jtj [nport][npar][npar] = J^T J with J = dr / dparams over all
 * npar external parameters (no bounds, no step).                           */
int ppf_gauss_eval(ppf_ctx* ctx, int32_t nport, int32_t nchan, int32_t nbin, int32_t ngauss,
                   const double* data /* [nport][nchan][nbin] */,
                   const double* freqs /* [nport][nchan] */,
                   const double* errs /* [nport][nchan] */,
                   const double* params /* [nport][npar] */,
                   const int32_t* code /* [nport][3]: loc, wid, amp; 0 power law, 1 linear */,
                   const double* nu_ref /* [nport] */, double* chi2 /* [nport] */,
                   double* jtr /* [nport][npar] */, double* jtj /* [nport][npar][npar] */);

/* status of a Gaussian-component fit (info[p][0]) */
#define PPF_GAUSS_FTOL 1      /* converged: MINPACK's ftol test */
#define PPF_GAUSS_XTOL 2      /* converged: MINPACK's xtol test */
#define PPF_GAUSS_BOTH 3      /* converged: both */
#define PPF_GAUSS_MAXFEV 5    /* evaluation cap reached */
#define PPF_GAUSS_SINGULAR -1 /* no step could be taken from the normal equations */
#define PPF_GAUSS_NONFINITE -2 /* the residual at the initial point is not finite */

/* ppf_gauss_fit_batch: Levenberg-Marquardt from init [nport][npar] over the
 * parameters with flags[p][q] != 0, the rest fixed.  Bounds are lmfit's
 * (pplib.py:1964-1988): tau >= 0, 0 <= wid <= 0.25, amp >= 0, imposed by
 * its MINUIT transforms on internal variables (lower: val = min - 1 +
 * sqrt(x^2 + 1); two-sided: val = min + (sin x + 1)(max - min) / 2); an
 * initial value outside its bounds is clipped.  Each iteration solves
 * (J^T J + lambda D^2) d = -J^T r by a Cholesky in fp64 with MINPACK's column
 * scaling D (running maximum of the column norms, 1 for a zero column) and
 * accepts the step by the gain ratio.  It stops by MINPACK's ftol / xtol
 * tests (scipy.optimize.leastsq's defaults are 1.49012e-8 for both; pass
 * them) or at max_nfev evaluations (0: 2000 (nfree + 1)).
 *   params [nport][npar]; param_errs [nport][npar] = lmfit's stderr with
 * scale_covar (sqrt(diag(inv(J^T J))) carried to the external values, times
 * sqrt(chi2 / dof)), 0 for fixed parameters and for all when J^T J is
 * singular; cov [nport][npar][npar] (may be NULL) the same covariance;
 * chi2 [nport]; info [nport][4] = {PPF_GAUSS_* status, evaluations made,
 * dof = nchan nbin - nfree, nfree}.  The call synchronises the stream once
 * per iteration.                                                           */
int ppf_gauss_fit_batch(ppf_ctx* ctx, int32_t nport, int32_t nchan, int32_t nbin, int32_t ngauss,
                        const double* data, const double* freqs, const double* errs,
                        const double* init /* [nport][npar] */,
                        const int32_t* flags /* [nport][npar] */, const int32_t* code,
                        const double* nu_ref, double ftol, double xtol, int32_t max_nfev,
                        double* params, double* param_errs, double* cov, double* chi2,
                        int32_t* info);

/* Joint fits of several receivers' portraits (fit_gaussian_portrait with
 * join_params, pplib.py:923-929, 1992-2001).  The rows of a portrait belong to
 * njoin groups (one per receiver; bands may overlap, so groups may interleave)
 * and the external vector has npar = 3 + 6 ngauss + 2 njoin entries: DC, tau,
 * the components, then phase_g [rot] and DM_g per group, then alpha (lmfit's
 * order).  Row n of group g = join_of[n] is the model row rotated as
 * rotate_data(row, phase_g, DM_g, P, f_n, nu_ref) does it: every harmonic k
 * of the model times exp(+2 pi i k theta_n), theta_n = phase_g + DM_g
 * dm_coef[n], the imaginary part at DC and Nyquist dropped after the product.
 * The caller passes dm_coef[n] = Dconst (f_n^-2 - nu_ref^-2) / P.  The model
 * is rotated, not the data: at the Nyquist harmonic the two are different
 * functions.  The join parameters are unbounded.  join_of [nport][nchan]
 * int32 in 0 .. njoin - 1 (PPF_ERR_INVALID otherwise, checked before the fit
 * reads it), dm_coef [nport][nchan] double; the other arguments, the results
 * and the guarantees are those of ppf_gauss_eval and ppf_gauss_fit_batch,
 * which are unchanged.
 *   Limits: 1 <= njoin <= 8 and 3 + 6 ngauss + 2 njoin <= 99
 * (PPF_ERR_UNSUPPORTED otherwise).                                          */
int ppf_gauss_eval_join(ppf_ctx* ctx, int32_t nport, int32_t nchan, int32_t nbin, int32_t ngauss,
                        int32_t njoin, const double* data, const double* freqs,
                        const double* errs, const double* params, const int32_t* code,
                        const double* nu_ref, const int32_t* join_of /* [nport][nchan] */,
                        const double* dm_coef /* [nport][nchan] */, double* chi2, double* jtr,
                        double* jtj);
int ppf_gauss_fit_join_batch(ppf_ctx* ctx, int32_t nport, int32_t nchan, int32_t nbin,
                             int32_t ngauss, int32_t njoin, const double* data,
                             const double* freqs, const double* errs, const double* init,
                             const int32_t* flags, const int32_t* code, const double* nu_ref,
                             const int32_t* join_of, const double* dm_coef, double ftol,
                             double xtol, int32_t max_nfev, double* params, double* param_errs,
                             double* cov, double* chi2, int32_t* info);

/* ---------------------------------------------------------------------- */
/* Fits across the channels of a row (ppfit_chanfit.hip): one wave per row, */
/* the whole fit inside one launch, no workspace.  1 <= n <= 16384 and      */
/* nrow >= 1 (PPF_ERR_INVALID otherwise).  A row's results are bitwise the  */
/* same whatever else shares the call.  Both are timed under PPF_K_GAUSS.   */
/* ---------------------------------------------------------------------- */

/* status of a row that cannot be fitted: fewer than 3 usable points, or a
 * usable point with a non-finite value (y; x in the line fit), nu <= 0 or
 * nu_ref <= 0.  Its results are NaN; the other rows are not disturbed.    */
#define PPF_CHANFIT_UNUSABLE -3

/* ppf_powlaw_fit_rows: pplib.fit_powlaw per row -- the model A (nu /
 * nu_ref)^alpha with the residual (y - model) / errs of fit_powlaw_function
 * (pplib.py:1204-1217), which the reference hands to lmfit's leastsq without
 * bounds.  y, errs, freqs [nrow][n]; nu_ref [nrow]; init [nrow][2] = A,
 * alpha.  A point whose errs is <= 0, NaN or infinite is left out: that is
 * how a zapped channel is passed.  The power is exp(alpha ln(nu / nu_ref))
 * in fp64.
 *   Levenberg-Marquardt with the analytic Jacobian under the rules of
 * ppf_gauss_fit_batch: the step from the 2 x 2 normal equations (J^T J +
 * lambda D^2) d = -J^T r with MINPACK's column scaling D, accepted by the
 * gain ratio; MINPACK's ftol / xtol tests (leastsq's defaults are
 * 1.49012e-8; pass them); max_nfev evaluations at most (0: 2000 * 3).
 *   out [nrow][6] = A, A_err, alpha, alpha_err, cov(A, alpha), chi2: errors
 * and covariance are lmfit's with scale_covar, inv(J^T J) chi2 / dof (zeros
 * when J^T J is singular).  info [nrow][4] = {status, evaluations made, dof
 * = n_used - 2, n_used}; status is PPF_GAUSS_FTOL / XTOL / BOTH (converged),
 * PPF_GAUSS_MAXFEV, PPF_GAUSS_SINGULAR, PPF_GAUSS_NONFINITE (the residual at
 * init is not finite) or PPF_CHANFIT_UNUSABLE.                             */
int ppf_powlaw_fit_rows(ppf_ctx* ctx, int32_t nrow, int32_t n, const double* y,
                        const double* errs, const double* freqs, const double* nu_ref,
                        const double* init, double ftol, double xtol, int32_t max_nfev,
                        double* out, int32_t* info);

/* ppf_line_fit_rows: np.polyfit(x, y, 1, w=w, cov=True) per row in closed
 * form, as pplib.fit_DM_to_freq_resids uses it (pplib.py:1804-1840): a and b
 * minimise sum (w_i (y_i - a x_i - b))^2.  x, y, w [nrow][n]; points with w
 * <= 0 or non-finite w are left out.  x and y are centred on their
 * w^2-weighted means before the slope is formed.
 *   out [nrow][8] = a, b, var(a), var(b), cov(a, b), sum (w r)^2, n_used,
 * status: the covariance of the normal equations times sum (w r)^2 / (n_used
 * - 2) (numpy >= 1.16; older ones divided by n - 4).  status is 0,
 * PPF_CHANFIT_UNUSABLE, or PPF_GAUSS_SINGULAR when every usable x is the
 * same; the first six entries of such a row are NaN.                       */
int ppf_line_fit_rows(ppf_ctx* ctx, int32_t nrow, int32_t n, const double* x, const double* y,
                      const double* w, double* out);

/* ppf_gauss_bank: the matched-filter bank of the automatic component search
 * (pplib.auto_gaussian_profiles).  For profile p, width w and bin j the
 * template g is the unit-amplitude component as the fit builds it --
 * gen_gaussian_profile([0, 0, loc_j, widths[w], 1.0], nbin) with loc_j the
 * centre of bin j, the same bin-centre wrap, |z| < 20 support and rescale
 * factor -- scattered by 1 / (1 + 2 pi i k taun[p]) when taun[p] != 0.  With
 * c = <resid[p], g> and gg = <g, g>: amp = c / gg and s2 = c^2 / (gg
 * errs[p]^2) where c > 0, else 0.  best[p] is the maximum of s2 over (w, j),
 * ties to the smaller width index, then the smaller bin; with no s2 > 0
 * best[p] is zeros and best_idx[p] is -1, -1.  c is computed as a circular
 * correlation on the spectra, gg by Parseval.
 *   Limits: nbin a power of two in [64, 8192], 1 <= nwid <= 64
 * (PPF_ERR_UNSUPPORTED otherwise); widths outside (0, 0.25] are
 * PPF_ERR_INVALID.  Scratch is workspace (ppf_set_workspace_limit splits the
 * call over profiles).  Results are bitwise reproducible and do not depend on
 * how many profiles share the call.                                        */
int ppf_gauss_bank(ppf_ctx* ctx, int32_t nprof, int32_t nbin, int32_t nwid,
                   const double* resid /* DEVICE [nprof][nbin] */,
                   const double* errs /* DEVICE [nprof], > 0 */,
                   const double* taun /* DEVICE [nprof], tau / nbin; 0 = unscattered */,
                   const double* widths /* HOST [nwid], FWHM in (0, 0.25] */,
                   double* s2 /* DEVICE [nprof][nwid][nbin], may be NULL */,
                   double* best /* DEVICE [nprof][4]: s2, loc, wid, amp */,
                   int32_t* best_idx /* DEVICE [nprof][2]: width index, bin; -1, -1 if none */);

/* B-spline (PCA) template rows (gen_spline_portrait, pplib.py:932-956, as
 * read_spline_model builds them, pplib.py:2961-2993): row r at freqs[r] is
 * mean_prof + sum_e splev(freqs[r], (t, c[e], k), ext=0) eigvec[:, e]
 * (FITPACK splev / fpbspl); neig == 0 tiles mean_prof.  When nbin_in !=
 * nbin the rows are resampled as scipy.signal.resample (rfft branch) and
 * rotated by 0.5 (1/nbin - 1/nbin_in) (rotate_portrait), both then in
 * [16, 8192].  t HOST [nknot], c HOST [neig][ncoef] (ncoef >=
 * nknot - k - 1), 1 <= k <= 5, neig <= 64; mean_prof [nbin_in], eigvec
 * [nbin_in][neig], freqs [nrow], out [nrow][nbin] on the device.          */
int ppf_spline_portraits(ppf_ctx* ctx, int32_t nrow, int32_t nbin_in, int32_t nbin, int32_t neig,
                         const double* mean_prof, const double* eigvec, int32_t nknot, int32_t k,
                         const double* t, const double* c, int32_t ncoef, const double* freqs,
                         double* out);

/* Instrumental-response convolution of template rows (get_TOAs with
 * add_instrumental_response, pptoas.py:387-393): out[r] = irfft(R_r *
 * rfft(in[r])) with R = instrumental_response_port_FT(nbin, freqs, DM, P,
 * wids, irf_types) (pptoaslib.py:145-179): the product over nw responses
 * (types HOST [nw]: 0 'rect' np.sinc(k wid), 1 'gauss' the normalised
 * Gaussian FT of FWHM wid [rot] <= 0.1388; wids HOST [nw], > 0) and, when
 * DM != 0, 'rect' of width 8.3e-6 chan_bw / (freqs[r] / 1e3)^3 / P (the
 * reference's formula: DM only switches it on).  chan_bw is the caller's
 * |freqs[1] - freqs[0]|.  in NULL: out receives R itself [nrow][nbin/2+1]. */
int ppf_instrumental_response_rows(ppf_ctx* ctx, int32_t nrow, int32_t nbin, const double* in,
                                   int32_t nw, const double* wids, const int32_t* types,
                                   double DM, double chan_bw, double P, const double* freqs,
                                   double* out);

/* tscrunch (load_data's arch.tscrunch(), pplib.py:2700) of fold-mode
 * subints: out[p][n][j] = sum_s w[s][n] data[s][p][n][j] / sum_s w[s][n]
 * (0 where the weights sum to 0), wsum[n] = sum_s w[s][n] (NULL: not
 * written).  data [nsub][npol][nchan][nbin], weights [nsub][nchan].      */
int ppf_tscrunch(ppf_ctx* ctx, int32_t nsub, int32_t npol, int32_t nchan, int32_t nbin,
                 const double* data, const double* weights, double* out, double* wsum);

/* PSRFITS samples to physical values (PSRCHIVE's load + pscrunch in
 * load_data, pplib.py:2670-2732): raw [nsub][npol][nchan][nbin] of
 * raw_type (ppfits.h PPFITS_RAW_*: 1 uint8, 2 int16, 3 float32), scl and
 * offs [nsub][npol][nchan] (DAT_SCL, DAT_OFFS); value = raw * scl + offs.
 * pmode 0 keeps every polarisation, 1 sums the first two (AA + BB), 2 takes
 * the first (Stokes I); out [nsub][pmode ? 1 : npol][nchan][nbin].
 * A fit needs no such copy of 16-bit samples: ppf_fit_portrait_batch_raw
 * reads them in its data pass.                                            */
int ppf_unpack_subints(ppf_ctx* ctx, int32_t nsub, int32_t npol, int32_t nchan, int32_t nbin,
                       int32_t raw_type, const void* raw, const double* scl, const double* offs,
                       int32_t pmode, double* out);

/* remove_baseline in place (load_data's arch.remove_baseline(),
 * pplib.py:2691; PSRCHIVE Integration::remove_baseline with its default
 * estimator): per subint s the total-intensity profile
 *   t[j] = sum_{n: w[s][n] != 0} w[s][n] sum_{p < ntot} data[s][p][n][j]
 * gives the off-pulse window [j0, j0 + width) (circular) of smallest sum,
 * first on ties; every profile data[s][p][n] then has its mean over that
 * window subtracted.  A window whose sum is NaN never wins; if no window
 * has an ordered sum (every sum NaN), the window starts at 0.
 * data [nsub][npol][nchan][nbin] (nbin <= 8192),
 * weights [nsub][nchan]; window [nsub] receives j0 (NULL: not written).
 * Callers pass width = floor(0.15 nbin), PSRCHIVE's default duty cycle.   */
int ppf_remove_baseline(ppf_ctx* ctx, int32_t nsub, int32_t npol, int32_t nchan, int32_t nbin,
                        int32_t ntot, int32_t width, double* data, const double* weights,
                        int32_t* window);

/* Per-profile S/N, load_data's SNRs[isub, ipol, ichan] =
 * Profile::snr() (pplib.py:2762-2770; get_TOAs weights guess_fit_freq with
 * them, pptoas.py:401).  Restated from PSRCHIVE's default "phase" S/N
 * estimator (PSRCHIVE is not in this image: PARITY UNPINNED):
 *   off-pulse window: the circular run of `width` bins with the smallest
 *     sum (first on ties; windows summed bin by bin from their start); a
 *     window whose sum is NaN never wins, and if no window has an ordered
 *     sum the window starts at 0 (a row with a NaN bin then has C = NaN
 *     and snr 0);
 *   m, v: mean and sample variance (n - 1) over that window;
 *   edges (cumulative-power peak): with y the profile minus m read
 *     circularly from the bin after the window, c its running sum and
 *     C = c[nbin - 1], rise = the first bin with c >= threshold C, fall =
 *     the first with c >= (1 - threshold) C;
 *   snr = (c[fall] - c[rise] + y[rise]) / sqrt(fall - rise + 1) / sqrt(v),
 *     0 when C <= 0 or v <= 0.
 * rows [nrow][nbin] (nbin <= 8192), out [nrow].  Callers pass width =
 * floor(0.15 nbin) and threshold 0.1.                                      */
int ppf_profile_snr(ppf_ctx* ctx, int32_t nrow, int32_t nbin, const double* rows, int32_t width,
                    double threshold, double* out);

/* out[r] = irfft(rfft(in[r]) e^{2 pi i k phase[r]} / (1 + 2 pi i k tau[r]))
 * (rotate_portrait_full of a scattered template, pptoas.py:1389-1397);
 * tau NULL = no scattering.                                              */
int ppf_scatter_rotate_rows(ppf_ctx* ctx, int32_t nrow, int32_t nbin, const double* in,
                            const double* phase, const double* tau, double* out);

/* Per-channel reduced chi2 of a fitted portrait, get_red_chi2 as
 * GetTOAs.get_channels_to_zap calls it (pplib.py:727-749, pptoas.py:1233):
 *   port  = irfft(rfft(data[r]) e^{2 pi i k phase[r]})
 *   model = scale[r] irfft(rfft(model[mrow]) / (1 + 2 pi i k tau[r]))
 *   out[r] = sum_j ((port_j - model_j) / errs[r])^2 / dof
 * evaluated in the Fourier domain (Parseval); mrow = model_row[r] (or r
 * when NULL), phase NULL = 0, tau NULL = no scattering.                  */
int ppf_resid_chi2_rows(ppf_ctx* ctx, int32_t nrow, int32_t nbin, const double* data,
                        const double* phase, const double* model, const int32_t* model_row,
                        const double* scale, const double* tau, const double* errs,
                        double dof, double* out);

/* out[r] = irfft(spec[r]) where spec is complex [nrow][nbin/2+1]           */
int ppf_irfft_rows(ppf_ctx* ctx, int32_t nrow, int32_t nbin, const double* spec,
                   double* out);

/* out[r] = get_noise_PS(in[r]) (frac=4)                                   */
int ppf_noise_rows(ppf_ctx* ctx, int32_t nrow, int32_t nbin, const double* in,
                   double* out);

/* out[r] = get_noise_PS(in[r], frac) for any frac > 1 (pplib.py:2227-2253):
 * the root of the mean power above harmonic int((1 - 1/frac) (nbin/2 + 1)).
 * ppf_noise_rows is its frac = 4 case.                                     */
int ppf_noise_rows_frac(ppf_ctx* ctx, int32_t nrow, int32_t nbin, double frac,
                        const double* in, double* out);

/* noise_out[r] = get_noise_fit(in[r], fact) (pplib.py:2255-2287): with
 * pows_k = |rfft(in[r])_k|^2 / nbin, k < NH = nbin/2 + 1, and kc = find_kc(pows)
 * as ppf_find_kc_rows (exp_dc, no weights) finds it,
 *   k_crit = fact kc;  if k_crit >= NH: k_crit = min(int(0.99 NH), k_crit)
 *   noise  = sqrt(mean(pows[int(k_crit):]))
 * kc_out [nrow] and idx_out [nrow] (either may be NULL) receive kc and the
 * flat index of the winning grid point.  fact > 0; nbin in [16, 8192].  A
 * row's outputs are bitwise the same whatever else shares the call.  Timed
 * under PPF_K_NOISE, like ppf_find_kc_rows.                                */
int ppf_noise_fit_rows(ppf_ctx* ctx, int32_t nrow, int32_t nbin, const double* in,
                       double fact, double* noise_out, int32_t* kc_out, int32_t* idx_out);

/* find_kc (pplib.py:1465-1495) on power spectra pows [nrow][n], 4 <= n <= 8193:
 * scipy.optimize.brute(Ns = 20, finish = None) of
 *   sum_k w_k (log10 pows_k - b f_a(k) - dc)^2,  w_k = 1 / errs_k^2 (errs [n],
 *   shared by the rows; NULL = 1)
 * over a_i = i (a_hi - a_lo) / 19 + a_lo, b_i = i (max d - min d) / 19,
 * dc_i = min d + i (max d - min d) / 19, d = log10 pows, i < 20:
 *   fn 0 (exp_dc):   f_a(k) = e^{-a k}, a in [1/n, 1];
 *                    kc = the first k with e^{-a k} < 0.005, or n - 1
 *   fn 1 (half_tri): f_a(k) = max(0, 1 - k / floor(a)), a in [1, n]; kc = floor(a)
 * idx_out (or NULL) = (ia 20 + ib) 20 + idc of the smallest value; among equal
 * values the lowest index, and the first NaN before any number, as
 * numpy.argmin: a row holding a zero, negative or non-finite power, or a
 * weight that is not finite, returns index 0.                              */
int ppf_find_kc_rows(ppf_ctx* ctx, int32_t nrow, int32_t n, const double* pows,
                     const double* errs, int32_t fn, int32_t* kc_out, int32_t* idx_out);

/* data[s][n] = irfft(rfft(model[n]) * e^{2 pi i k phase[s][n]})
 *              + sigma * N(0,1)[Philox4x32-10(seed; bin pair, n, s + sub0)] */
int ppf_synth_portraits(ppf_ctx* ctx, int32_t nsub, int32_t nchan, int32_t nbin,
                        const double* model, const double* phase, double sigma,
                        uint64_t seed, int64_t sub0, double* data);

/* fp64 values to 16-bit PSRFITS samples, the inverse of ppf_unpack_subints:
 * data [nsub][npol][nchan][nbin] -> raw (int16, native byte order) with scl
 * and offs [nsub][npol][nchan], value ~ raw * scl + offs.  Per row, with lo
 * and hi its exact minimum and maximum:
 *   offs = (float)(0.5 (lo + hi))
 *   scl  = the smallest float32 >= max(hi - offs, offs - lo) / 32767 (fp64)
 *   raw  = rint((x - offs) / scl) in fp64, ties to even
 * so |raw| <= 32767 without a clamp and |raw scl + offs - x| <= scl / 2 up
 * to fp64 rounding.  scl and offs are fp64 values exactly representable in
 * float32 (the file stores them as E).  A constant row takes scl = 1, offs =
 * (float)lo, raw = 0.  A row with a non-finite sample is stored as zeros
 * (scl 1, offs 0) and the call returns PPF_ERR_INVALID.  The call waits for
 * the stream (it returns that status).                                     */
int ppf_pack_subints(ppf_ctx* ctx, int32_t nsub, int32_t npol, int32_t nchan, int32_t nbin,
                     const double* data, int16_t* raw, double* scl, double* offs);

/* ppf_synth_portraits with polarisations, amplitudes and per-channel noise:
 * data[s][p][n] = amp[s][n] irfft(rfft(model[n]) e^{2 pi i k phase[s][n]})
 *                 + sigma[n] N(0,1)[Philox4x32-10(seed; bin pair,
 *                                                  n + nchan p, s + sub0)]
 * model [nchan][nbin], phase and amp [nsub][nchan], sigma [nchan].  The
 * result does not depend on how the subints are split into calls (sub0);
 * with npol = 1, amp = 1 and one sigma it is bitwise ppf_synth_portraits'.
 * Output, one of:
 *   data [nsub][npol][nchan][nbin] fp64 (raw, scl, offs NULL; no wait), or
 *   raw, scl, offs (data NULL): those rows quantised exactly as
 *   ppf_pack_subints quantises them, its status and its wait included.  For
 *   a power-of-two nbin >= 64 one kernel makes and quantises each row in
 *   LDS, so 2 bytes per sample reach HBM; other nbin write the fp64 rows to
 *   workspace (PPF_ERR_NOMEM above the workspace limit) and pack them.    */
int ppf_fake_subints(ppf_ctx* ctx, int32_t nsub, int32_t npol, int32_t nchan, int32_t nbin,
                     const double* model, const double* phase, const double* amp,
                     const double* sigma, uint64_t seed, int64_t sub0, double* data, int16_t* raw,
                     double* scl, double* offs);

#ifdef __cplusplus
}
#endif
#endif /* PPFIT_H */
