"""numpy / scipy restatement of the wavelet smoothing the device code builds
(DESIGN.md section 9), written from that definition and independent of the
device code: the undecimated db8 transform with periodic extension as plain
loops over the 16 taps with modular indices, the reference's threshold and
objective, and scipy.optimize.brute with its default fmin finish for the
search.  It is not PyWavelets and is not pinned against it.

Every function takes dtype (np.float64 or np.longdouble) so that the
objective's own rounding can be measured.
"""
import numpy as np
import scipy.optimize as opt

# db8 scaling filter, PyWavelets' rec_lo order, to 17 significant digits (the
# minimum-phase factor of P(y) = sum_{k<8} C(7+k, k) y^k)
H = np.array([
    0.054415842243104008, 0.31287159091429995, 0.67563073629728976, 0.58535468365420673,
    -0.015829105256349306, -0.28401554296154691, 0.00047248457391328279, 0.12874742662047847,
    -0.017369301001807547, -0.044088253930794755, 0.013981027917398282, 0.0087460940474057766,
    -0.0048703529934515741, -0.00039174037337694705, 0.00067544940645056933,
    -0.00011747678412476953])
G = np.array([(-1) ** k * H[15 - k] for k in range(16)])

# the named test profiles: (nbin, sigma, seeds)
CASES = [(64, 0.05, (1, 2, 3)), (128, 0.05, (1, 2, 3)), (256, 0.02, (1, 2, 3)),
         (2048, 0.02, (1,))]


def case_list():
    return [(nbin, seed, sigma) for nbin, sigma, seeds in CASES for seed in seeds]


def named_profile(nbin, seed, sigma):
    rng = np.random.default_rng(seed)
    t = np.arange(nbin) / nbin
    return (np.exp(-0.5 * ((t - 0.3) / 0.04) ** 2) + 0.4 * np.exp(-0.5 * ((t - 0.45) / 0.02) ** 2)
            + sigma * rng.standard_normal(nbin))


def _filt(x, f, step, sign):
    """y[n] = sum_k f[k] x[(n + sign step k) mod N]."""
    n = len(x)
    idx = np.arange(n)
    y = np.zeros_like(x)
    for k in range(16):
        y = y + x.dtype.type(f[k]) * x[(idx + sign * step * k) % n]
    return y


_LAST_SWT = [None, None]  # the forward transform does not depend on the threshold


def swt(x, nlevel):
    """(a_L, [d_1 .. d_L])."""
    if len(x) % (1 << nlevel):
        raise ValueError("nbin=%d is not a multiple of 2^%d" % (len(x), nlevel))
    key = (x.dtype.str, nlevel, x.tobytes())
    if _LAST_SWT[0] == key:
        return _LAST_SWT[1]
    a, ds = x, []
    for j in range(1, nlevel + 1):
        s = 1 << (j - 1)
        ds.append(_filt(a, G, s, 1))
        a = _filt(a, H, s, 1)
    _LAST_SWT[:] = [key, (a, ds)]
    return a, ds


def iswt(a, ds):
    for j in range(len(ds), 0, -1):
        s = 1 << (j - 1)
        a = (_filt(a, H, s, -1) + _filt(ds[j - 1], G, s, -1)) / a.dtype.type(2)
    return a


def threshold(c, lam, threshtype):
    if threshtype == "hard":
        return np.where(np.abs(c) < lam, c.dtype.type(0), c)
    if threshtype == "soft":
        return np.sign(c) * np.maximum(np.abs(c) - lam, c.dtype.type(0))
    raise ValueError(threshtype)


def lam_of(a, ds, fact, nbin):
    t = a.dtype.type
    med = np.median(np.abs(np.concatenate([a, ds[-1]])))
    return t(fact) * (med / t(0.6745)) * np.sqrt(t(2) * np.log(t(nbin)))


def wavelet_smooth(prof, nlevel=5, threshtype="hard", fact=1.0, dtype=np.float64, details=False):
    """The smoothed profile; with details also lambda and every |coefficient|
    (a_L, then d_1 .. d_L)."""
    x = np.asarray(prof, dtype=dtype)
    a, ds = swt(x, nlevel)
    lam = lam_of(a, ds, fact, len(x))
    y = iswt(threshold(a, lam, threshtype), [threshold(d, lam, threshtype) for d in ds])
    if details:
        return y, lam, np.abs(np.concatenate([a] + ds))
    return y


def rfft_any(x):
    """rfft; numpy's FFT is double only, so a direct DFT in a wider type."""
    if x.dtype == np.float64:
        return np.fft.rfft(x)
    n = len(x)
    k = np.arange(n // 2 + 1)
    t = x.dtype.type
    ang = (t(8) * np.arctan(t(1)) / t(n)) * (np.outer(k, np.arange(n)) % n).astype(x.dtype)
    return (np.cos(ang) - 1j * np.sin(ang)) @ x


def get_noise(prof):
    """get_noise_PS: the mean of the top quarter of the power spectrum."""
    x = np.asarray(prof)
    F = rfft_any(x)
    pw = (F.real ** 2 + F.imag ** 2) / x.dtype.type(len(x))
    kc = int((1 - 1.0 / 4) * len(pw))
    return np.sqrt(np.mean(pw[kc:]))


def get_red_chi2(data, model):
    data, model = np.asarray(data), np.asarray(model)
    return np.sum(((data - model) / get_noise(data)) ** 2) / data.dtype.type(len(data))


def fit_wavelet_smooth_function(fact, prof, nlevel, threshtype="hard", rchi2_tol=0.1,
                                dtype=np.float64, full=False):
    fact = float(np.ravel(fact)[0])
    x = np.asarray(prof, dtype=dtype)
    s = wavelet_smooth(x, nlevel, threshtype, fact, dtype)
    F = rfft_any(s)[1:]
    signal = np.sum(F.real ** 2 + F.imag ** 2)
    if signal:
        noise = get_noise(s) * np.sqrt(x.dtype.type(len(s)) / x.dtype.type(2))
        snr = signal / noise if noise else np.inf
    else:
        snr = x.dtype.type(0)
    red_chi2 = get_red_chi2(x, s)
    if abs(red_chi2 - 1) > rchi2_tol:
        snr = x.dtype.type(0)
    return (-snr, red_chi2) if full else -snr


def smart_smooth(prof, try_nlevels=None, rchi2_tol=0.1, threshtype="hard", full=False):
    """The smoothed profile; with full a dict of the search's results."""
    prof = np.asarray(prof, dtype=np.float64)
    nbin = len(prof)
    ident = dict(smooth=prof, nlevel=0, fact=0.0, red_chi2=0.0, zeroed=False, fun_vals=None)
    if try_nlevels == 0 or nbin % 2:
        return ident if full else prof
    if np.modf(np.log2(nbin))[0] != 0.0:
        try_nlevels = 1
    elif try_nlevels is None:
        try_nlevels = int(np.log2(nbin))
    if not np.any(prof):
        ident["smooth"] = np.zeros(nbin)
        return ident if full else ident["smooth"]
    fun_vals, fact_mins = np.zeros(try_nlevels), np.zeros(try_nlevels)
    for ilevel in range(try_nlevels):
        res = opt.brute(fit_wavelet_smooth_function, ranges=[(0.0, 3.0)],
                        args=(prof, ilevel + 1, threshtype, rchi2_tol), Ns=30, full_output=True)
        fact_mins[ilevel] = res[0][0]
        fun_vals[ilevel] = res[1]
    imin = int(fun_vals.argmin())
    fact = fact_mins[imin]
    smooth = wavelet_smooth(prof, imin + 1, threshtype, fact)
    red_chi2 = get_red_chi2(prof, smooth)
    zeroed = bool(abs(red_chi2 - 1.0) > rchi2_tol)
    if zeroed:
        smooth = smooth * 0.0
    if full:
        return dict(smooth=smooth, nlevel=imin + 1, fact=fact, red_chi2=red_chi2, zeroed=zeroed,
                    fun_vals=fun_vals)
    return smooth


_SMART = {}


def named_smart(nbin, seed, sigma, threshtype="hard"):
    """smart_smooth(full=True) of a named profile, computed once per process
    and shared by the tests (do not modify the result)."""
    key = (nbin, seed, sigma, threshtype)
    if key not in _SMART:
        _SMART[key] = smart_smooth(named_profile(nbin, seed, sigma), threshtype=threshtype,
                                   full=True)
    return _SMART[key]


def objective_rounding(levels_of, nbins=(64, 128)):
    """The largest relative difference between the objective in float64 and
    in np.longdouble over the named profiles of nbins, the levels
    levels_of(nbin) and the 30 grid points; also the float64 values
    {(nbin, seed, level): (objectives [30], red_chi2 [30])}."""
    worst, vals = 0.0, {}
    for nbin, seed, sigma in case_list():
        if nbin not in nbins:
            continue
        prof = named_profile(nbin, seed, sigma)
        for level in levels_of(nbin):
            f64 = [fit_wavelet_smooth_function(g * (3.0 / 29), prof, level, full=True)
                   for g in range(30)]
            f80 = [fit_wavelet_smooth_function(g * (3.0 / 29), prof, level, dtype=np.longdouble)
                   for g in range(30)]
            for (a, _), b in zip(f64, f80):
                d = abs(a - float(b))
                worst = max(worst, d / abs(a) if a else d)
            vals[(nbin, seed, level)] = (np.array([float(a) for a, _ in f64]),
                                         np.array([float(rc) for _, rc in f64]))
    return worst, vals
