"""numpy + scipy restatement of the automatic Gaussian-component search
(pplib.auto_gaussian_profiles, ppf_gauss_bank): the yardstick of
tests/test_gpu_auto_gauss.py and of tests/golden/make_golden_auto_gauss.py.

  bank()   the matched-filter bank from its definition: one template per
           (width, bin) from pplib.gen_gaussian_profile, c = <resid, g>, gg =
           <g, g>, s2 = c^2 / (gg err^2) where c > 0;
  fit()    scipy's MINPACK (leastsq) on the yardstick's residual with its
           analytic Jacobian (tests/golden/make_golden_ppgauss.py) at
           leastsq's default tolerances, one channel under the "111" code;
  bank_fft()  the same map as a circular correlation (the fast CPU form);
  auto()   the greedy pursuit with the search's rules;
  truth()  the fit started from the true parameters at ftol = xtol = 1e-13.

Runs on the CPU; nothing here touches the device.
"""
import functools
import importlib.util
import os

import numpy as np

from pulseportraiture_amd import pplib

HERE = os.path.dirname(os.path.abspath(__file__))
WID_MAX = 0.25
EDGE = 1e-6


def _yardstick():
    spec = importlib.util.spec_from_file_location(
        "make_golden_ppgauss", os.path.join(HERE, "golden", "make_golden_ppgauss.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


Y = _yardstick()


def noise_ps(profile):
    """get_noise_PS (pplib.py:2227-2253): the top quarter of the power spectrum."""
    nbin = len(profile)
    ps = np.abs(np.fft.rfft(profile)) ** 2 / nbin
    kc = int(0.75 * len(ps))
    return float(np.sqrt(np.mean(ps[kc:])))


def widths(nbin, nwid=16):
    return np.geomspace(2.0 / nbin, WID_MAX, nwid)


@functools.lru_cache(maxsize=8)
def _templates(nbin, wids, taun):
    """[nwid, nbin (bin of the centre), nbin]: the unit-amplitude component of
    every (width, bin) exactly as the fit builds it."""
    locs = pplib.get_bin_centers(nbin)
    return np.array([[pplib.gen_gaussian_profile([0.0, taun * nbin, loc, w, 1.0], nbin)
                      for loc in locs] for w in wids])


def bank(resid, err, taun, wids):
    """s2 [nwid, nbin], best = (s2, loc, wid, amp) and idx = (width index,
    bin) of its maximum (first in width-major order; zeros and -1, -1 when no
    correlation is positive)."""
    resid = np.asarray(resid, dtype=np.float64)
    nbin = len(resid)
    T = _templates(nbin, tuple(float(w) for w in wids), float(taun))
    c = T @ resid
    gg = np.sum(T * T, axis=-1)
    s2 = np.where(c > 0.0, c * c / (gg * err * err), 0.0)
    if not np.any(s2 > 0.0):
        return s2, np.zeros(4), (-1, -1)
    w, j = np.unravel_index(np.argmax(s2), s2.shape)
    best = np.array([s2[w, j], pplib.get_bin_centers(nbin)[j], wids[w], c[w, j] / gg[w, j]])
    return s2, best, (int(w), int(j))


def bank_fft(resid, err, taun, wids):
    """bank() as a circular correlation: one template per width (bin 0's),
    turned by the FFT.  The fast form a CPU user would write; it is what
    tools/time_auto_gauss.py clocks, and it equals bank() to rounding."""
    resid = np.asarray(resid, dtype=np.float64)
    nbin = len(resid)
    locs = pplib.get_bin_centers(nbin)
    g0 = np.array([pplib.gen_gaussian_profile([0.0, taun * nbin, locs[0], w, 1.0], nbin)
                   for w in wids])
    c = np.fft.irfft(np.fft.rfft(resid)[None] * np.conj(np.fft.rfft(g0, axis=-1)), n=nbin,
                     axis=-1)
    gg = np.sum(g0 * g0, axis=-1)[:, None]
    s2 = np.where(c > 0.0, c * c / (gg * err * err), 0.0)
    if not np.any(s2 > 0.0):
        return s2, np.zeros(4), (-1, -1)
    w, j = np.unravel_index(np.argmax(s2), s2.shape)
    return s2, np.array([s2[w, j], locs[j], wids[w], c[w, j] / gg[w, 0]]), (int(w), int(j))


def _problem(profile, err, params, fit_scattering):
    """The yardstick's Problem of a profile fit: one channel at nu_ref under
    the linear code with the slopes fixed at 0 (fit_gaussian_profile)."""
    params = np.asarray(params, dtype=np.float64)
    ngauss = (len(params) - 2) // 3
    par, fl = np.zeros(3 + 6 * ngauss), np.zeros(3 + 6 * ngauss, dtype=int)
    par[:2], fl[:2] = params[:2], [1, int(fit_scattering)]
    for k in range(3):
        par[2 + 2 * k:-1:6], fl[2 + 2 * k:-1:6] = params[2 + k::3], 1
    keep = np.sort(np.concatenate([[0, 1]] + [np.arange(2 + 2 * k, len(par) - 1, 6)
                                             for k in range(3)]))
    pr = Y.Problem("111", np.asarray(profile, dtype=np.float64)[None], np.array([float(err)]),
                   np.ones(1), 1.0, par, fl)
    return pr, keep.astype(int)


def _solved(pr, keep, x, cov_x, info, ier):
    p = pr.external(x)
    chi2 = float(np.sum(info["fvec"] ** 2))
    dof = pr.data.size - len(pr.free)
    sig = np.zeros(len(p))
    if cov_x is not None:
        g = Y.dexternal(x, pr.kind[pr.free])
        sig[pr.free] = np.sqrt(np.diag(cov_x) * g * g * chi2 / dof)
    return dict(p=p[keep], sig=sig[keep], chi2=chi2, dof=dof, ier=ier, nfev=info["nfev"])


def fit(profile, err, params, fit_scattering=False):
    """leastsq with the analytic Jacobian at its default ftol and xtol."""
    from scipy.optimize import leastsq
    pr, keep = _problem(profile, err, params, fit_scattering)
    x, cov_x, info, _, ier = leastsq(pr.resid, pr.x0(), Dfun=pr.jac, full_output=True)
    return _solved(pr, keep, x, cov_x, info, ier)


def truth(profile, err, params, fit_scattering=False):
    """The fit from the true parameters at ftol = xtol = 1e-13."""
    from scipy.optimize import leastsq
    pr, keep = _problem(profile, err, params, fit_scattering)
    x, cov_x, info, _, ier = leastsq(pr.resid, pr.x0(), Dfun=pr.jac, full_output=True,
                                     ftol=1e-13, xtol=1e-13)
    return _solved(pr, keep, x, cov_x, info, ier)


def accept(ier, chi2_new, chi2_old, params, nbin):
    wids, amps = np.asarray(params[3::3]), np.asarray(params[4::3])
    return bool(ier in (1, 2, 3, 4) and chi2_new + 3.0 * np.log(nbin) < chi2_old
                and np.all(np.abs(amps) > EDGE) and np.all(wids > EDGE)
                and np.all(wids < WID_MAX - EDGE))


def auto(profile, err, max_ngauss=8, tau=0.0, fit_scattering=False, min_snr=5.0, nwid=16,
         bank=bank):
    """The search.  Returns p (DC, tau, loc, wid, amp per component in order
    of discovery), sig, chi2, dof, ngauss and history; every history entry
    carries `margin`, the relative s2 margin of the best cell over every
    other cell, and `resid`, the residual its bank saw."""
    profile = np.asarray(profile, dtype=np.float64)
    nbin = len(profile)
    wids = widths(nbin, nwid)
    dc = np.mean(profile)  # the least-squares fit of the zero-component model
    p, sig = np.array([dc, float(tau)]), np.zeros(2)
    resid = profile - dc
    chi2, dof, ngauss, history = float(np.sum((resid / err) ** 2)), nbin - 1, 0, []
    while True:
        if ngauss >= max_ngauss:
            history.append(dict(s2=np.nan, candidate=None, chi2_old=chi2, chi2_new=np.nan,
                                accepted=False, stop="max_ngauss", margin=np.inf, resid=resid))
            break
        s2, best, idx = bank(resid, err, p[1] / nbin, wids)
        flat = np.sort(s2.ravel())
        margin = (flat[-1] - flat[-2]) / flat[-1] if flat[-1] > 0.0 else np.inf
        if best[0] < min_snr ** 2:
            history.append(dict(s2=best[0], candidate=None, chi2_old=chi2, chi2_new=np.nan,
                                accepted=False, stop="min_snr", margin=margin, resid=resid))
            break
        r = fit(profile, err, np.concatenate([p, best[1:]]), fit_scattering)
        ok = accept(r["ier"], r["chi2"], chi2, r["p"], nbin)
        history.append(dict(s2=best[0], candidate=best[1:].copy(), chi2_old=chi2,
                            chi2_new=r["chi2"], accepted=ok, stop=None if ok else "rejected",
                            margin=margin, resid=resid, idx=idx))
        if not ok:
            break
        p, sig, chi2, dof, ngauss = r["p"], r["sig"], r["chi2"], r["dof"], ngauss + 1
        resid = profile - pplib.gen_gaussian_profile(p, nbin)
    return dict(p=p, sig=sig, chi2=chi2, dof=dof, ngauss=ngauss, history=history)


def match_order(p, p_true):
    """p's components matched to p_true's by nearest loc (on the circle), each
    true component taking one of p's: component n of the result is p's
    component order[n]."""
    p, p_true = np.asarray(p, dtype=np.float64), np.asarray(p_true, dtype=np.float64)
    comps, left, order = p[2:].reshape(-1, 3), list(range((len(p) - 2) // 3)), []
    for loc in p_true[2::3]:
        d = [abs((comps[i, 0] - loc + 0.5) % 1.0 - 0.5) for i in left]
        order.append(left.pop(int(np.argmin(d))))
    return order


def reorder(v, order):
    """A profile-layout vector (two leading entries, three per component)
    with its components in the given order."""
    v = np.asarray(v, dtype=np.float64)
    return np.concatenate([v[:2], v[2:].reshape(-1, 3)[order].ravel()])


def delta(p, q):
    """p - q for profile-layout vectors, the locs compared on the circle."""
    d = np.asarray(p, dtype=np.float64) - np.asarray(q, dtype=np.float64)
    d[2::3] = (d[2::3] + 0.5) % 1.0 - 0.5
    return d
