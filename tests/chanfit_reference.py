"""numpy / scipy restatement of the fits across channels (include/ppfit.h,
ppf_powlaw_fit_rows and ppf_line_fit_rows): the CPU yardstick of
tests/test_gpu_chanfit.py.

- the power law: scipy.optimize.leastsq on the residual (y - A (nu /
  nu_ref)**alpha) / errs over the usable points, as lmfit's minimize runs it
  for pplib.fit_powlaw (forward differences, default tolerances: `reference`),
  and the same restarted with the analytic Jacobian and ftol = xtol = 1e-15
  (`truth`).  Covariances are lmfit's with scale_covar: cov_x chi2 / dof.
- the line: np.polyfit(x, y, 1, w=w, cov=True) over the usable points, and the
  same closed form in np.longdouble.
"""
import numpy as np
from scipy.optimize import leastsq

Dconst = 0.000241 ** -1
ALPHAS = (-4.4, -1.6, 0.0, 2.0)
SNRS = (5.0, 50.0, 500.0)
NS = (3, 5, 64, 65, 200, 513)
NREP = 6  # rows per (alpha, S/N): 72 rows per n


def usable(e):
    with np.errstate(invalid="ignore"):
        return np.isfinite(e) & (e > 0.0)


def powlaw_resid(p, y, e, f, nu_ref):
    return (y - p[0] * (f / nu_ref) ** p[1]) / e


def powlaw_jac(p, y, e, f, nu_ref):
    m = (f / nu_ref) ** p[1]
    return np.column_stack([-m / e, -p[0] * m * np.log(f / nu_ref) / e])


def _bunch(x, cov_x, y, e, f, nu_ref, nfev):
    r = powlaw_resid(x, y, e, f, nu_ref)
    chi2, dof = float(r @ r), len(y) - 2
    cov = cov_x * chi2 / dof
    return dict(amp=x[0], alpha=x[1], amp_err=cov[0, 0] ** 0.5, alpha_err=cov[1, 1] ** 0.5,
                cov=cov[0, 1], chi2=chi2, dof=dof, n_used=len(y), nfev=nfev)


def powlaw_reference(y, e, f, nu_ref, x0):
    """The reference's own configuration on the usable points of one row."""
    ok = usable(e)
    a = (y[ok], e[ok], f[ok], nu_ref)
    x, cov_x, info, _, _ = leastsq(powlaw_resid, np.array(x0, dtype=float), args=a,
                                   full_output=True)
    return _bunch(x, cov_x, *a, nfev=info["nfev"])


def powlaw_truth(y, e, f, nu_ref, x0):
    """leastsq restarted from the reference's end point with the analytic
    Jacobian and ftol = xtol = 1e-15, twice."""
    ok = usable(e)
    a = (y[ok], e[ok], f[ok], nu_ref)
    x = np.array([powlaw_reference(y, e, f, nu_ref, x0)[k] for k in ("amp", "alpha")])
    for _ in range(2):
        x, cov_x, info, _, _ = leastsq(powlaw_resid, x, args=a, Dfun=powlaw_jac, ftol=1e-15,
                                       xtol=1e-15, gtol=0.0, full_output=True)
    return _bunch(x, cov_x, *a, nfev=info["nfev"])


def mask_rows(e, rng):
    """One tenth of each row's points left out where n > 5, by every value that
    leaves a point out (0, negative, NaN, inf); on the first rows the masks sit
    on a lane's first point (index 0) and last point (the last index, and the
    last multiple of 64: lane 0's last)."""
    nrow, n = e.shape
    if n <= 5:
        return e
    bad = (0.0, -1.0, np.nan, np.inf)
    nmask = max(n // 10, 1)
    for r in range(nrow):
        idx = rng.choice(n, nmask, replace=False)
        if r % 4 == 0:
            idx[0] = 0
        if r % 4 == 1:
            idx[0] = n - 1
        if r % 4 == 2:
            idx[0] = 64 * ((n - 1) // 64)
        for k, i in enumerate(idx):
            e[r, i] = bad[(r + k) % 4]
    return e


def powlaw_inputs(n, seed=20240607):
    """The 72 rows of check 1 at n points: sorted uniform frequencies in [700,
    2300] MHz, nu_ref 1500, A uniform in [0.5, 20], errors A / SNR * U(0.5, 2),
    alpha and S/N over ALPHAS x SNRS."""
    rng = np.random.default_rng(seed + n)
    rows = [(al, snr) for al in ALPHAS for snr in SNRS for _ in range(NREP)]
    nrow = len(rows)
    f = np.sort(rng.uniform(700.0, 2300.0, (nrow, n)), axis=1)
    A = rng.uniform(0.5, 20.0, nrow)
    al = np.array([r[0] for r in rows])
    snr = np.array([r[1] for r in rows])
    e = A[:, None] / snr[:, None] * rng.uniform(0.5, 2.0, (nrow, n))
    y = A[:, None] * (f / 1500.0) ** al[:, None] + e * rng.standard_normal((nrow, n))
    e = mask_rows(e, rng)
    return dict(y=y, errs=e, freqs=f, nu_ref=np.full(nrow, 1500.0), amp=A, alpha=al, snr=snr)


def line_inputs(n, nrow=24, seed=777):
    """Rows of check 2: nu linear in [1100, 1900] MHz, y = Dconst dDM nu**-2 +
    offset + noise with per-point errors, one tenth of the points left out.
    Returns x = nu**-2, y, the errors and w = errs**-2 (fit_DM_to_freq_resids'
    weight, 0 at the points left out)."""
    rng = np.random.default_rng(seed + n)
    nu = np.tile(np.linspace(1100.0, 1900.0, n), (nrow, 1))
    dDM = rng.uniform(-2e-3, 2e-3, nrow)
    off = rng.uniform(-1e-5, 1e-5, nrow)
    e = rng.uniform(0.5e-6, 4e-6, (nrow, n))
    y = Dconst * dDM[:, None] * nu ** -2 + off[:, None] + e * rng.standard_normal((nrow, n))
    e = mask_rows(e, rng)
    with np.errstate(all="ignore"):
        w = np.where(usable(e), e, np.inf) ** -2
    return dict(freqs=nu, x=nu ** -2, y=y, errs=e, w=w, dDM=dDM, offset=off)


def line_polyfit(x, y, w):
    """np.polyfit with its covariance on the usable points of one row:
    a, b, var(a), var(b), cov(a, b), sum (w r)^2."""
    ok = usable(w)
    p, V = np.polyfit(x[ok], y[ok], 1, w=w[ok], cov=True)
    r = w[ok] * (y[ok] - (p[0] * x[ok] + p[1]))
    return np.array([p[0], p[1], V[0, 0], V[1, 1], V[0, 1], r @ r])


def line_truth(x, y, w):
    """The same closed form in np.longdouble (centred normal equations, the
    covariance scaled by sum (w r)^2 / (n_used - 2))."""
    ok = usable(w)
    L = np.longdouble
    x, y, W = x[ok].astype(L), y[ok].astype(L), w[ok].astype(L) ** 2
    sw = W.sum()
    xm, ym = (W * x).sum() / sw, (W * y).sum() / sw
    sxx = (W * (x - xm) ** 2).sum()
    a = (W * (x - xm) * (y - ym)).sum() / sxx
    b = ym - a * xm
    s2 = (W * (y - a * x - b) ** 2).sum()
    fac = s2 / (len(x) - 2)
    return np.array([a, b, fac / sxx, fac * (1 / sw + xm * xm / sxx), -fac * xm / sxx, s2],
                    dtype=L)


def dm_bunch(freqs, resids, errs):
    """fit_DM_to_freq_resids' fields from np.polyfit on the usable points of
    one row (pplib.py:1804-1840; dof counts the usable points)."""
    ok = usable(errs)
    x, w = freqs ** -2.0, np.where(ok, errs, np.inf) ** -2.0
    a, b, va, vb, cov, _ = line_polyfit(x, resids, w)
    with np.errstate(all="ignore"):
        nu_ref = (-b / a) ** -0.5
        nu_ref_err = (((nu_ref ** 2) / 4.0) * ((va / a ** 2) + (vb / b ** 2) -
                                               (2 * cov / (a * b)))) ** 0.5
    residuals = resids - (a * x + b)
    chi2 = ((residuals[ok] / errs[ok]) ** 2).sum()
    dof = int(ok.sum()) - 2
    return dict(DM=a / Dconst, DM_err=va ** 0.5 / Dconst, offset=b, offset_err=vb ** 0.5,
                nu_ref=nu_ref, nu_ref_err=nu_ref_err, ab_cov=cov, residuals=residuals, chi2=chi2,
                dof=dof, red_chi2=chi2 / dof)
