"""pplib drop-in: constants, templates, TOA output and the GPU-backed utilities.

Hot-path numerics (rfft/irfft, noise, rotation, FFTFIT search, portrait fits)
run in libppfit.so via ``engine``; this module keeps the reference's call
signatures (pplib.py) and its host-side producers/consumers:
Gaussian-component templates (read_model / gen_gaussian_portrait,
pplib.py:752-1046, 2834-2959) and the .tim writer (pplib.py:3386-3509).
"""
import pickle
import sys
import time

import numpy as np

# pplib.py:44-119 --------------------------------------------------------------
Dconst_exact = 4.148808e3
Dconst_trad = 0.000241 ** -1
Dconst = Dconst_trad
scattering_alpha = -4.0
use_get_noise = True
default_noise_method = "PS"
F0_fact = 0
wid_max = 0.25
default_model = "000"
binshift = 1.0
RCSTRINGS = {"-1": "INFEASIBLE: Infeasible (low > up).",
             "0": "LOCALMINIMUM: Local minima reach (|pg| ~= 0).",
             "1": "FCONVERGED: Converged (|f_n-f_(n-1)| ~= 0.)",
             "2": "XCONVERGED: Converged (|x_n-x_(n-1)| ~= 0.)",
             "3": "MAXFUN: Max. number of function evaluations reach.",
             "4": "LSFAIL: Linear search failed.",
             "5": "CONSTANT: All lower bounds are equal to the upper bounds.",
             "6": "NOPROGRESS: Unable to progress.",
             "7": "USERABORT: User requested end of minimization."}


class DataBunch(dict):
    """dict with attribute access (pplib.py:125-136)."""

    def __init__(self, **kwds):
        dict.__init__(self, kwds)
        self.__dict__ = self


def _engine():
    from .engine import get_engine
    return get_engine()


# ---------------------------------------------------------------------------
# Gaussian-component templates (host-side input producer)
# ---------------------------------------------------------------------------
def get_bin_centers(nbin, lo=0.0, hi=1.0):
    """pplib.py:671-684."""
    lo, hi = np.double(lo), np.double(hi)
    d = hi - lo
    return np.double(np.linspace(lo + d / (nbin * 2), hi - d / (nbin * 2), nbin))


def gaussian_profile(nbin, loc, wid, norm=False, abs_wid=False, zeroout=True):
    """Peak-1 Gaussian on bin centres, pplib.py:770-825."""
    if abs_wid:
        wid = abs(wid)
    if not wid > 0.0:
        if wid == 0.0 or (wid < 0.0 and zeroout):
            return np.zeros(nbin, "d")
        if not wid < 0.0:
            return 0
    sigma = wid / (2 * np.sqrt(2 * np.log(2)))
    mean = loc % 1.0
    x = get_bin_centers(nbin)
    if mean < 0.5:
        x = np.where(x > mean + 0.5, x - 1.0, x)
    else:
        x = np.where(x < mean - 0.5, x + 1.0, x)
    zs = (x - mean) / sigma
    out = np.zeros(nbin, "d")
    ok = np.fabs(zs) < 20.0
    out[ok] = np.exp(-0.5 * zs[ok] ** 2.0) / (sigma * np.sqrt(2 * np.pi))
    if norm or np.max(abs(out)) == 0.0:
        return out
    i = out.argmax()
    z = (x[i] - loc) / sigma
    return np.exp(-0.5 * z ** 2.0) / out[i] * out


def scattering_times(tau, alpha, freqs, nu_tau):
    """pplib.py:4055-4059."""
    return tau * (freqs / nu_tau) ** alpha


def scattering_profile_FT(tau, nbin, binshift=binshift):
    """(1 + 2 pi i k tau)^-1, pplib.py:4061-4084."""
    nharm = nbin // 2 + 1
    if tau == 0.0:
        return np.ones(nharm)
    return (1.0 + 2 * np.pi * 1.0j * np.arange(nharm) * tau) ** -1


def scattering_portrait_FT(taus, nbin, binshift=binshift):
    """pplib.py:4086-4101."""
    taus = np.atleast_1d(taus)
    nharm = nbin // 2 + 1
    if not np.any(taus):
        return np.ones([len(taus), nharm])
    return np.array([scattering_profile_FT(t, nbin) for t in taus])


def gen_gaussian_profile(params, nbin):
    """DC + sum of Gaussians, optionally scattered; pplib.py:827-851."""
    ngauss = (len(params) - 2) // 3
    model = np.zeros(nbin, dtype="d") + params[0]
    for ig in range(ngauss):
        loc, wid, amp = params[2 + ig * 3:5 + ig * 3]
        model += amp * gaussian_profile(nbin, loc, wid)
    if params[1] != 0.0:
        # n=nbin: the reference's irfft (pplib.py:850) drops a bin at odd
        # nbin; the same for even nbin
        model = np.fft.irfft(scattering_profile_FT(float(params[1]) / nbin, nbin)
                             * np.fft.rfft(model), n=nbin)
    return model


def power_law_evolution(freqs, nu_ref, parameter, index):
    """pplib.py:996-1011."""
    return np.exp(np.outer(np.log(freqs) - np.log(nu_ref), index) +
                  np.outer(np.ones(len(freqs)), np.log(parameter)))


def linear_evolution(freqs, nu_ref, parameter, slope):
    """pplib.py:1013-1028."""
    return np.outer(freqs - nu_ref, slope) + np.outer(np.ones(len(freqs)), parameter)


def evolve_parameter(freqs, nu_ref, parameter, evol_parameter, code):
    """pplib.py:1030-1046."""
    fn = {"0": power_law_evolution, "1": linear_evolution}[code]
    return fn(freqs, nu_ref, parameter, evol_parameter)


def gen_gaussian_portrait(model_code, params, scattering_index, phases, freqs, nu_ref,
                          join_ichans=[], P=None):
    """Frequency-evolving Gaussian portrait, pplib.py:853-930.  With
    join_ichans (lists of channels, one per receiver) the last 2 len(join_ichans)
    entries of params are a phase [rot] and a DM per list, by which its rows
    are rotated as rotate_data does it (numpy's rfft on the host); P [sec] is
    needed then."""
    params = np.asarray(params, dtype=float)
    njoin = len(join_ichans)
    if njoin:
        join_params, params = params[-2 * njoin:], params[:-2 * njoin]
    ref = np.array([params[0], params[1] * 0.0] + list(params[2::2]))
    tau = params[1]
    nbin, nchan = len(phases), len(freqs)
    gp = np.empty([nchan, len(ref)])
    gp[:, 0] = ref[0]
    gp[:, 1] = ref[1]
    gp[:, 2::3] = evolve_parameter(freqs, nu_ref, ref[2::3], params[3::6], model_code[0])
    gp[:, 3::3] = evolve_parameter(freqs, nu_ref, ref[3::3], params[5::6], model_code[1])
    gp[:, 4::3] = evolve_parameter(freqs, nu_ref, ref[4::3], params[7::6], model_code[2])
    port = np.array([gen_gaussian_profile(gp[i], nbin) for i in range(nchan)])
    if tau != 0.0:
        taus = scattering_times(float(tau) / nbin, scattering_index, freqs, nu_ref)
        # n=nbin as the device's k_rotate_rows<RowAny> (pplib.py:921 has no n=
        # and returns nbin - 1 bins at odd nbin); the same for even nbin
        port = np.fft.irfft(scattering_portrait_FT(taus, nbin) *
                            np.fft.rfft(port, axis=-1), n=nbin, axis=-1)
    for ij in range(njoin):
        ic = np.asarray(join_ichans[ij], dtype=int)
        theta = join_rotations(join_params[2 * ij], join_params[2 * ij + 1], P,
                               np.asarray(freqs, dtype=float)[ic], nu_ref)
        phasor = np.exp(2.0j * np.pi * np.outer(theta, np.arange(nbin // 2 + 1)))
        port[ic] = np.fft.irfft(np.fft.rfft(port[ic], axis=-1) * phasor, n=nbin, axis=-1)
    return port


def join_dm_coef(P, freqs, nu_ref):
    """d theta / d DM of a row at freqs: Dconst (f^-2 - nu_ref^-2) / P [rot per
    cm**-3 pc] (rotate_data, pplib.py:2389-2413)."""
    return Dconst * (np.asarray(freqs, dtype=float) ** -2.0 - nu_ref ** -2.0) / P


def join_rotations(phase, DM, P, freqs, nu_ref):
    """The rotation [rot] rotate_data(rows, phase, DM, P, freqs, nu_ref) applies
    to each row."""
    freqs = np.asarray(freqs, dtype=float)
    if DM == 0.0:
        return np.full(len(freqs), float(phase))
    return phase + Dconst * DM / P * (freqs ** -2.0 - nu_ref ** -2.0)


def join_groups(join_ichans, nchan):
    """join_of [nchan]: the index of the list in join_ichans that holds each
    channel.  The device fit takes one group per row: channels in no list
    (left unrotated by the reference) or in several are refused."""
    join_of = np.full(nchan, -1, dtype=np.int32)
    count = np.zeros(nchan, dtype=int)
    for ij, ic in enumerate(join_ichans):
        ic = np.asarray(ic, dtype=int)
        join_of[ic] = ij
        np.add.at(count, ic, 1)
    if np.any(count != 1):
        raise NotImplementedError("join_params whose lists do not hold every channel exactly "
                                  "once are not supported: the device fit takes one join group "
                                  "per row")
    return join_of


def join_row_rotations(join_ichans, join_params, P, freqs, nu_ref):
    """The rotation [rot] of every row of a portrait at freqs [nchan] under the
    join parameters (phase_g, DM_g per list of join_ichans); 0 for a channel
    in no list."""
    freqs = np.asarray(freqs, dtype=float)
    theta = np.zeros(len(freqs))
    for ij, ic in enumerate(join_ichans):
        ic = np.asarray(ic, dtype=int)
        theta[ic] = join_rotations(join_params[2 * ij], join_params[2 * ij + 1], P, freqs[ic],
                                   nu_ref)
    return theta


def rotate_join_rows(rows, join_ichans, join_params, P, freqs, nu_ref, sign=1.0):
    """rows [nchan, nbin] with the channels of join_ichans[g] rotated as
    rotate_data(rows, sign phase_g, sign DM_g, P, freqs, nu_ref) does it, in
    one device call (ppf_rotate_rows)."""
    theta = sign * join_row_rotations(join_ichans, join_params, P, freqs, nu_ref)
    return _engine().rotate_rows(np.asarray(rows, dtype=np.float64), theta).cpu().numpy()


def read_model(modelfile, phases=None, freqs=None, P=None, quiet=False):
    """Read a .gmodel (and build the portrait when phases/freqs given), pplib.py:2873-2959."""
    read_only = phases is None and freqs is None
    comps = []
    name = code = None
    nu_ref = dc = tau = alpha = 0.0
    fit_dc = fit_tau = fit_alpha = 0
    with open(modelfile, "rb") as fh:  # a pickled spline model is not UTF-8 text
        lines = fh.read().decode("latin-1").splitlines()
    for line in lines:
        info = line.split()
        if not info:
            continue
        key = info[0]
        try:
            if key == "MODEL":
                name = info[1]
            elif key == "CODE":
                code = info[1]
            elif key == "FREQ":
                nu_ref = np.float64(info[1])
            elif key == "DC":
                dc, fit_dc = np.float64(info[1]), int(info[2])
            elif key == "TAU":
                tau, fit_tau = np.float64(info[1]), int(info[2])
            elif key == "ALPHA":
                alpha, fit_alpha = np.float64(info[1]), int(info[2])
            elif key[:4] == "COMP":
                comps.append(line)
        except IndexError:
            pass
    if name is None or code is None:
        # what the reference's read_model raises on a non-.gmodel file (its
        # unassigned locals), which get_TOAs takes as "spline model"
        # (pptoas.py:375-378)
        raise UnboundLocalError("%s is not a .gmodel file" % modelfile)
    ngauss = len(comps)
    params = np.zeros(ngauss * 6 + 2)
    flags = np.zeros(len(params))
    params[0], params[1] = dc, tau
    flags[0], flags[1] = fit_dc, fit_tau
    for ig, comp in enumerate(comps):
        f = comp.split()
        params[2 + ig * 6:8 + ig * 6] = [np.float64(v) for v in f[1::2]]
        flags[2 + ig * 6:8 + ig * 6] = [int(v) for v in f[2::2]]
    if read_only:
        return (name, code, nu_ref, ngauss, params, flags, alpha, fit_alpha)
    nbin = len(phases)
    if params[1] != 0:
        if P is None:
            print("Need period P for non-zero scattering value TAU.")
            return 0
        params[1] *= nbin / P
    model = gen_gaussian_portrait(code, params, alpha, phases, freqs, nu_ref)
    return (name, ngauss, model)


def gen_gaussian_portraits_device(model_code, params, scattering_index, nbin, freqs, nu_ref,
                                  join_ichans=[], P=None):
    """gen_gaussian_portrait (pplib.py:853-930) for rows of frequencies
    ([..., nchan]) in one device call (ppf_gaussian_portraits); returns a
    numpy array [..., nchan, nbin].  params[1] (TAU) in bins, as there.  With
    join_ichans the rows are then rotated by the join parameters at the end
    of params (ppf_rotate_rows)."""
    from .engine import get_engine
    eng = get_engine()
    njoin = len(join_ichans)
    if not njoin:
        return eng.gaussian_portraits(model_code, params, scattering_index, nbin, freqs,
                                      nu_ref).cpu().numpy()
    params = np.asarray(params, dtype=float)
    join_params, params = params[-2 * njoin:], params[:-2 * njoin]
    freqs = np.asarray(freqs, dtype=float)
    port = eng.gaussian_portraits(model_code, params, scattering_index, nbin, freqs, nu_ref)
    theta = np.array([join_row_rotations(join_ichans, join_params, P, f, nu_ref)
                      for f in freqs.reshape(-1, freqs.shape[-1])])
    out = eng.rotate_rows(port.reshape(-1, nbin), theta.ravel())
    return out.cpu().numpy().reshape(freqs.shape + (nbin,))


def read_model_device(modelfile, nbin, freqs, P=None, quiet=False):
    """read_model(modelfile, phases, freqs, P) (pplib.py:2873-2959) with the
    portrait built on the device for every row of freqs ([..., nchan]): the
    .gmodel parse, TAU *= nbin / P, then gen_gaussian_portraits_device.
    Returns (name, ngauss, model [..., nchan, nbin])."""
    name, code, nu_ref, ngauss, params, flags, alpha, fit_alpha = read_model(modelfile,
                                                                             quiet=True)
    params = np.array(params, dtype=float)
    if params[1] != 0:
        if P is None:
            print("Need period P for non-zero scattering value TAU.")
            return 0
        params[1] *= nbin / P
    return name, ngauss, gen_gaussian_portraits_device(code, params, alpha, nbin, freqs, nu_ref)


# ---------------------------------------------------------------------------
# Gaussian-component fits (ppgauss): lmfit's leastsq on the device
# ---------------------------------------------------------------------------
def _row_errs(errs, shape):
    """The per-row error of the reference's errs array (one value per sample,
    pplib.py:1945): [nchan] values when every row is constant."""
    e = np.asarray(errs, dtype=np.float64)
    if e.ndim == len(shape) - 1 or e.ndim == 0:
        return np.broadcast_to(e, shape[:-1]).copy()
    e = np.broadcast_to(e, shape)
    if np.any(e != e[..., :1]):
        raise NotImplementedError("errs that vary along a profile are not supported: the "
                                  "device fit takes one error per channel")
    return e[..., 0].copy()


def _gauss_bunch(out, i, quiet, title, njoin=0):
    from ._lib import GAUSS_STATUS
    status, nfev, dof = (int(v) for v in out["info"][i, :3])
    params, errs = out["params"][i], out["param_errs"][i]
    lm = DataBunch(status=status, message=GAUSS_STATUS.get(status, "unknown"), nfev=nfev,
                   covar=out["cov"][i], success=status in (1, 2, 3))
    chi2 = float(out["chi2"][i])
    if not quiet:
        print("---------------------------------------------------------------")
        print(title)
        print("---------------------------------------------------------------")
        print("status:", lm.message)
        print("Gaussians:", (len(params) - 3 - 2 * njoin) // 6)
        print("DoF:", dof)
        print("reduced chi-sq: %.2g" % (chi2 / dof))
        print("---------------------------------------------------------------")
    # (with join parameters fitted_params ends with them, pplib.py:2024-2031)
    return DataBunch(lm_results=lm, fitted_params=params[:-1].copy(), fit_errs=errs[:-1].copy(),
                     scattering_index=params[-1], scattering_index_err=errs[-1], chi2=chi2,
                     dof=dof)


def fit_gaussian_portraits(model_codes, datas, init_params, scattering_indices, errs, fit_flags,
                           fit_scattering_indices, phases, freqs, nu_refs, join_params=[],
                           Ps=None, quiet=True, ftol=1.49012e-8, xtol=1.49012e-8, max_nfev=0):
    """fit_gaussian_portrait for a list of portraits of one shape in one
    device call (ppf_gauss_fit_batch): every argument but phases is a list
    (or an array with a leading portrait axis).  Returns a list of DataBunch.

    join_params: one [join_ichanxs, params, flags] per portrait (the
    reference's, pplib.py:1992-2001) with the same number of lists of channels
    in each, and Ps the periods [sec]: a joint fit of several receivers
    (ppf_gauss_fit_join_batch).  fitted_params and fit_errs then end with the
    2 njoin join entries."""
    if len(join_params):
        return _fit_gaussian_portraits_join(
            model_codes, datas, init_params, scattering_indices, errs, fit_flags,
            fit_scattering_indices, phases, freqs, nu_refs, join_params, Ps, quiet, ftol, xtol,
            max_nfev)
    n = len(datas)
    data = np.stack([np.asarray(d, dtype=np.float64) for d in datas])
    if data.ndim != 3 or data.shape[-1] != len(phases):
        raise ValueError("portraits of one shape [nchan, nbin = len(phases)] per call")
    par = np.array([np.append(np.asarray(p, dtype=np.float64), float(a))
                    for p, a in zip(init_params, scattering_indices)])
    fl = np.array([np.append(np.asarray(f) != 0, bool(fa))
                   for f, fa in zip(fit_flags, fit_scattering_indices)])
    er = np.stack([_row_errs(e, data.shape[1:]) for e in errs])
    out = _engine().gauss_fit(data, np.stack([np.asarray(f, dtype=np.float64) for f in freqs]),
                              er, par, fl, [str(c) for c in model_codes],
                              np.asarray(nu_refs, dtype=np.float64), ftol, xtol, max_nfev)
    out = {k: v.cpu().numpy() for k, v in out.items()}
    return [_gauss_bunch(out, i, quiet, "Gaussian Portrait Fit") for i in range(n)]


def _fit_gaussian_portraits_join(model_codes, datas, init_params, scattering_indices, errs,
                                 fit_flags, fit_scattering_indices, phases, freqs, nu_refs,
                                 join_params, Ps, quiet, ftol, xtol, max_nfev):
    """fit_gaussian_portraits with join parameters."""
    n = len(datas)
    if len(join_params) != n:
        raise ValueError("join_params: one [join_ichanxs, params, flags] per portrait")
    njoin = len(join_params[0][0])
    if any(len(jp[0]) != njoin for jp in join_params):
        raise ValueError("one number of join groups per call")
    data = np.stack([np.asarray(d, dtype=np.float64) for d in datas])
    if data.ndim != 3 or data.shape[-1] != len(phases):
        raise ValueError("portraits of one shape [nchan, nbin = len(phases)] per call")
    nchan = data.shape[1]
    join_of = np.stack([join_groups(jp[0], nchan) for jp in join_params])
    if Ps is None or len(Ps) != n or any(P is None for P in Ps):
        raise ValueError("join_params need the period P [sec] of every portrait")
    fr = np.stack([np.asarray(f, dtype=np.float64) for f in freqs])
    par = np.array([np.concatenate([np.asarray(p, dtype=np.float64),
                                    np.asarray(jp[1], dtype=np.float64), [float(a)]])
                    for p, jp, a in zip(init_params, join_params, scattering_indices)])
    fl = np.array([np.concatenate([np.asarray(f) != 0, np.asarray(jp[2]) != 0, [bool(fa)]])
                   for f, jp, fa in zip(fit_flags, join_params, fit_scattering_indices)])
    er = np.stack([_row_errs(e, data.shape[1:]) for e in errs])
    dm_coef = np.stack([join_dm_coef(P, f, nu) for P, f, nu in zip(Ps, fr, nu_refs)])
    out = _engine().gauss_fit_join(data, fr, er, par, fl, [str(c) for c in model_codes],
                                   np.asarray(nu_refs, dtype=np.float64), join_of, dm_coef, njoin,
                                   ftol, xtol, max_nfev)
    out = {k: v.cpu().numpy() for k, v in out.items()}
    return [_gauss_bunch(out, i, quiet, "Gaussian Portrait Fit", njoin) for i in range(n)]


def fit_gaussian_portrait(model_code, data, init_params, scattering_index, errs, fit_flags,
                          fit_scattering_index, phases, freqs, nu_ref, join_params=[], P=None,
                          quiet=True):
    """Fit evolving Gaussian components to a portrait (pplib.py:1924-2052) on
    the device: lmfit's leastsq with its bounds (tau >= 0, 0 <= wid <=
    wid_max, amp >= 0) and an analytic Jacobian.  Returns the reference's
    DataBunch; lm_results is a record of status, message, nfev, covar and
    success.  errs [nchan, nbin] has to be constant along each row.
    join_params = [join_ichanxs, params, flags] and the period P [sec] fit a
    phase and a DM per list of channels alongside (pplib.py:1992-2001)."""
    joined = len(join_params) > 0
    return fit_gaussian_portraits([model_code], [data], [init_params], [scattering_index], [errs],
                                  [fit_flags], [fit_scattering_index], phases, [freqs], [nu_ref],
                                  [join_params] if joined else [], [P] if joined else None,
                                  quiet)[0]


def profile_fit_flags(nparam, fit_flags=None, fit_scattering=False):
    """The flags of DC, tau, (loc, wid, amp) per component from
    fit_gaussian_profile's convention (pplib.py:1868-1873): fit_flags holds
    DC and the component parameters, tau follows fit_scattering."""
    if fit_flags is None:
        flags = [True] * nparam
        flags[1] = bool(fit_scattering)
        return flags
    return [bool(fit_flags[0]), bool(fit_scattering)] + [bool(fit_flags[i])
                                                         for i in range(1, nparam - 1)]


def _fit_gaussian_profiles(datas, init_params, errs, fit_flags=None, fit_scattering=False):
    """fit_gaussian_profile's solver call for profiles of one length and
    component count, in one device call: (fitted_params, fit_errs, portrait
    DataBunch) per profile."""
    datas = [np.asarray(d, dtype=np.float64) for d in datas]
    nbin = len(datas[0])
    pars, fls, es = [], [], []
    for data, init, err in zip(datas, init_params, errs):
        init = np.asarray(init, dtype=np.float64)
        nparam = len(init)
        ngauss = (nparam - 2) // 3
        flags = profile_fit_flags(nparam, fit_flags, fit_scattering)
        par, fl = np.zeros(2 + 6 * ngauss), np.zeros(2 + 6 * ngauss, dtype=bool)
        par[:2], fl[:2] = init[:2], flags[:2]
        for k in range(3):
            par[2 + 2 * k::6], fl[2 + 2 * k::6] = init[2 + k::3], flags[2 + k::3]
        pars.append(par)
        fls.append(fl)
        es.append(_row_errs((np.asarray(err, dtype=np.float64) + np.zeros(nbin))[None],
                            (1, nbin)))
    n = len(datas)
    fgps = fit_gaussian_portraits(["111"] * n, [d[None] for d in datas], pars, [0.0] * n, es, fls,
                                  [False] * n, get_bin_centers(nbin), [np.ones(1)] * n, [1.0] * n,
                                  quiet=True)
    keep = np.sort(np.concatenate([[0, 1]] + [np.arange(2 + 2 * k, len(pars[0]), 6)
                                             for k in range(3)])).astype(int)
    return [(fgp.fitted_params[keep], fgp.fit_errs[keep], fgp) for fgp in fgps]


def fit_gaussian_profile(data, init_params, errs, fit_flags=None, fit_scattering=False,
                         quiet=True):
    """Fit Gaussian components to a profile (pplib.py:1842-1922): the
    portrait solver with one channel at freq = nu_ref and the evolution
    parameters fixed at 0 under the linear code, where the value is the
    parameter exactly.  Returns fitted_params, fit_errs, residuals, chi2, dof."""
    data = np.asarray(data, dtype=np.float64)
    ngauss = (len(init_params) - 2) // 3
    fitted, fit_errs, fgp = _fit_gaussian_profiles([data], [init_params], [errs], fit_flags,
                                                   fit_scattering)[0]
    residuals = data - gen_gaussian_profile(fitted, len(data))
    if not quiet:
        print("---------------------------------------------------------------")
        print("Multi-Gaussian Profile Fit Results")
        print("---------------------------------------------------------------")
        print("status:", fgp.lm_results.message)
        print("Gaussians:", ngauss)
        print("DoF:", fgp.dof)
        print("reduced chi-sq: %.2f" % (fgp.chi2 / fgp.dof))
        print("residuals mean: %.3g" % np.mean(residuals))
        print("residuals std.: %.3g" % np.std(residuals))
        print("---------------------------------------------------------------")
    return DataBunch(fitted_params=fitted, fit_errs=fit_errs, residuals=residuals, chi2=fgp.chi2,
                     dof=fgp.dof, lm_results=fgp.lm_results)


# ---------------------------------------------------------------------------
# The automatic component search: a headless stand-in for ppgauss's
# interactive GaussianSelector (ppgauss.py:374-640)
# ---------------------------------------------------------------------------
AUTO_GAUSS_WID_MAX = 0.25  # the fit's upper bound on a width (pplib.py:1976)
AUTO_GAUSS_MAX = 16        # PPF_K_GAUSS: components in one fit
AUTO_GAUSS_EDGE = 1e-6     # a fitted amp or wid this close to a bound is on it


def auto_gaussian_widths(nbin, nwid=16, wid_max=AUTO_GAUSS_WID_MAX):
    """The FWHMs of the filter bank: two bins up to the fit's bound."""
    return np.geomspace(2.0 / nbin, wid_max, nwid)


def auto_gaussian_accept(status, chi2_new, chi2_old, params, nbin, wid_max=AUTO_GAUSS_WID_MAX):
    """Whether a refit with one more component is kept: it converged, it
    pays for its three parameters by the BIC, and no amplitude or width sits
    on a bound (where lmfit's errors mean nothing)."""
    wids, amps = np.asarray(params[3::3]), np.asarray(params[4::3])
    return bool(status in (1, 2, 3)
                and chi2_new + 3.0 * np.log(nbin) < chi2_old
                and np.all(np.abs(amps) > AUTO_GAUSS_EDGE)
                and np.all(wids > AUTO_GAUSS_EDGE)
                and np.all(wids < wid_max - AUTO_GAUSS_EDGE))


def auto_gaussian_profiles(profiles, errs=None, max_ngauss=8, tau=0.0, fit_scattering=False,
                           min_snr=5.0, nwid=16, quiet=True):
    """Find and fit the Gaussian components of profiles [nprof, nbin] with no
    starting values: a greedy matched-filter pursuit.  It starts from zero
    components, DC at the profile's mean (the fitted constant).  Each stage finds the
    most significant unit-amplitude component in every profile's residual
    (ppf_gauss_bank, one device call), appends it and refits DC and all
    components (tau [bin] too when fit_scattering) in one batched
    Levenberg-Marquardt call.  A profile stops when nothing reaches min_snr,
    at max_ngauss components, or when the refit is not accepted
    (auto_gaussian_accept); it then keeps its previous fit.  errs=None takes
    get_noise of each profile.

    Returns one DataBunch per profile: fitted_params (DC, tau, then loc, wid,
    amp per component in order of discovery), fit_errs, chi2, dof, ngauss,
    residuals, lm_results (None with no component) and history -- per stage
    s2, candidate, chi2_old, chi2_new, accepted and stop."""
    if max_ngauss > AUTO_GAUSS_MAX:
        raise ValueError("max_ngauss=%d: at most %d components in a fit"
                         % (max_ngauss, AUTO_GAUSS_MAX))
    profs = [np.asarray(p, dtype=np.float64) for p in profiles]
    nprof = len(profs)
    if not nprof:
        return []
    nbin = len(profs[0])
    if any(p.ndim != 1 or len(p) != nbin for p in profs):
        raise ValueError("profiles of one length per call")
    if errs is None:
        errs = [get_noise(p) for p in profs]
    errs = np.broadcast_to(np.asarray(errs, dtype=np.float64), (nprof,)).copy()
    widths = auto_gaussian_widths(nbin, nwid)
    eng = _engine()
    out = []
    for p, e in zip(profs, errs):
        dc = np.mean(p)  # the least-squares fit of the zero-component model
        resid = p - dc
        out.append(DataBunch(fitted_params=np.array([dc, float(tau)]),
                             fit_errs=np.array([e / np.sqrt(nbin), 0.0]),
                             chi2=float(np.sum((resid / e) ** 2)), dof=nbin - 1, ngauss=0,
                             residuals=resid, lm_results=None, history=[]))
    active = list(range(nprof))
    while active:
        run = []
        for i in active:
            b = out[i]
            if b.ngauss >= max_ngauss:
                b.history.append(DataBunch(s2=np.nan, candidate=None, chi2_old=b.chi2,
                                           chi2_new=np.nan, accepted=False, stop="max_ngauss"))
            else:
                run.append(i)
        if not run:
            break
        best, _ = eng.gauss_bank(np.stack([out[i].residuals for i in run]), errs[run],
                                 np.array([out[i].fitted_params[1] / nbin for i in run]), widths)
        best = best.cpu().numpy()
        fit = []
        for i, (s2, loc, wid, amp) in zip(run, best):
            if s2 < min_snr ** 2:
                out[i].history.append(DataBunch(s2=float(s2), candidate=None,
                                                chi2_old=out[i].chi2, chi2_new=np.nan,
                                                accepted=False, stop="min_snr"))
            else:
                fit.append((i, float(s2), np.array([loc, wid, amp])))
        active = []
        if not fit:
            break
        res = _fit_gaussian_profiles(
            [profs[i] for i, _, _ in fit],
            [np.concatenate([out[i].fitted_params, c]) for i, _, c in fit],
            [errs[i] for i, _, _ in fit], None, fit_scattering)
        for (i, s2, cand), (fitted, fit_errs, fgp) in zip(fit, res):
            b = out[i]
            ok = auto_gaussian_accept(fgp.lm_results.status, fgp.chi2, b.chi2, fitted, nbin)
            b.history.append(DataBunch(s2=s2, candidate=cand, chi2_old=b.chi2, chi2_new=fgp.chi2,
                                       accepted=ok, stop=None if ok else "rejected"))
            if not ok:
                continue
            b.fitted_params, b.fit_errs, b.chi2, b.dof = fitted, fit_errs, fgp.chi2, fgp.dof
            b.lm_results = fgp.lm_results
            b.ngauss += 1
            b.residuals = profs[i] - gen_gaussian_profile(fitted, nbin)
            active.append(i)
    if not quiet:
        for i, b in enumerate(out):
            print("profile %d: %d Gaussians, chi-sq %.6g, DoF %d, stopped by %s"
                  % (i, b.ngauss, b.chi2, b.dof, b.history[-1].stop))
    return out


def auto_gaussian_profile(profile, errs=None, max_ngauss=8, tau=0.0, fit_scattering=False,
                          min_snr=5.0, nwid=16, quiet=True):
    """auto_gaussian_profiles for one profile."""
    return auto_gaussian_profiles([profile], None if errs is None else [errs], max_ngauss, tau,
                                  fit_scattering, min_snr, nwid, quiet)[0]


# ---------------------------------------------------------------------------
# B-spline (PCA) templates: ppspline.py models (host reader, device builder)
# ---------------------------------------------------------------------------
class _SplineUnpickler(pickle.Unpickler):
    """Unpickler for ppspline model files (ppspline.py:206-228: a list of
    name, source, datafile, mean_prof, eigvec and tck) that resolves only
    numpy's array reconstruction: any other global in the file raises
    UnpicklingError, so loading a model executes nothing it names."""

    _ALLOWED = {("numpy.core.multiarray", "_reconstruct"),
                ("numpy._core.multiarray", "_reconstruct"),
                ("numpy.core.multiarray", "scalar"), ("numpy._core.multiarray", "scalar"),
                ("numpy", "ndarray"), ("numpy", "dtype"),
                ("_codecs", "encode"),  # protocol-2 bytes from Python 3
                ("__builtin__", "bytes"), ("builtins", "bytes")}  # ... and empty ones

    def find_class(self, module, name):
        if (module, name) not in self._ALLOWED:
            raise pickle.UnpicklingError("spline model: global %s.%s is not allowed"
                                         % (module, name))
        if name in ("ndarray", "dtype"):
            return getattr(np, name)
        if module == "_codecs":
            import codecs
            return codecs.encode
        if name == "bytes":
            return bytes
        try:
            from numpy._core import multiarray
        except ImportError:  # numpy 1.x
            from numpy.core import multiarray
        return getattr(multiarray, name)


def load_spline_model_file(modelfile):
    """(modelname, source, datafile, mean_prof, eigvec, tck) of a ppspline
    model: its Python-2 (or 3) pickle through _SplineUnpickler (latin-1 for
    Python-2 strings), or an .npz holding the same fields."""
    if str(modelfile).endswith(".npz"):
        z = np.load(modelfile, allow_pickle=False)
        tck = [z["t"], list(z["c"]), int(z["k"])]
        return (str(z["modelname"]), str(z["source"]), str(z["datafile"]), z["mean_prof"],
                z["eigvec"], tck)
    with open(modelfile, "rb") as fh:
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", DeprecationWarning)
            obj = _SplineUnpickler(fh, encoding="latin1").load()
    modelname, source, datafile, mean_prof, eigvec, tck = obj
    return modelname, source, datafile, np.asarray(mean_prof), np.asarray(eigvec), tck


def gen_spline_portrait(mean_prof, freqs, eigvec, tck, nbin=None):
    """gen_spline_portrait (pplib.py:932-956) on the device: FITPACK splev of
    the projections at freqs, eigvec . proj + mean_prof, and the resample +
    rotate when nbin != len(mean_prof) (ppf_spline_portraits).  Returns a
    numpy array [nchan, nbin]."""
    from .engine import get_engine
    eigvec = np.asarray(eigvec)
    return get_engine().spline_portraits(mean_prof, eigvec, tck, np.atleast_1d(freqs),
                                         nbin).cpu().numpy()


def read_spline_model(modelfile, freqs=None, nbin=None, quiet=False):
    """read_spline_model (pplib.py:2961-2993): the model tuple, or (name,
    portrait at freqs) built on the device."""
    if not quiet:
        print("Reading model from %s..." % modelfile)
    modelname, source, datafile, mean_prof, eigvec, tck = load_spline_model_file(modelfile)
    if freqs is None:
        return modelname, source, datafile, mean_prof, eigvec, tck
    return modelname, gen_spline_portrait(mean_prof, freqs, eigvec, tck, nbin)


def write_model(filename, name, model_code, nu_ref, model_params, fit_flags, alpha,
                fit_alpha, append=False, quiet=False):
    """pplib.py:2834-2871 (same text layout)."""
    with open(filename, "a" if append else "w") as out:
        out.write("MODEL   %s\n" % name)
        out.write("CODE    %s\n" % model_code)
        out.write("FREQ    %.5f\n" % nu_ref)
        out.write("DC     % .8f %d\n" % (model_params[0], fit_flags[0]))
        out.write("TAU    % .8f %d\n" % (model_params[1], fit_flags[1]))
        out.write("ALPHA  % .3f      %d\n" % (alpha, fit_alpha))
        for ig in range((len(model_params) - 2) // 6):
            comp = model_params[2 + ig * 6:8 + ig * 6]
            fc = fit_flags[2 + ig * 6:8 + ig * 6]
            line = (ig + 1,) + tuple(np.array(list(zip(comp, fc))).ravel())
            out.write("COMP%02d % .8f %d  % .8f %d  % .8f %d  % .8f %d  % .8f %d  % .8f %d\n"
                      % line)
    if not quiet:
        print("%s written." % filename)


# ---------------------------------------------------------------------------
# Scalar helpers (host)
# ---------------------------------------------------------------------------
def phase_transform(phi, DM, nu_ref1=np.inf, nu_ref2=np.inf, P=None, mod=False):
    """pplib.py:2592-2616."""
    if P is None:
        P, mod = 1.0, False
    out = phi + (Dconst * DM * P ** -1 * (nu_ref2 ** -2.0 - nu_ref1 ** -2.0))
    if mod:
        out = np.where(abs(out) >= 0.5, out % 1, out)
        out = np.where(out >= 0.5, out - 1.0, out)
        if not out.shape:
            out = np.float64(out)
    return out


def guess_fit_freq(freqs, SNRs=None):
    """pplib.py:2618-2632."""
    freqs = np.asarray(freqs, dtype=float)
    nu0 = (freqs.min() + freqs.max()) * 0.5
    if SNRs is None:
        SNRs = np.ones(len(freqs))
    return nu0 + np.sum((freqs - nu0) * SNRs * freqs ** -2) / np.sum(SNRs * freqs ** -2)


def DM_delay(DM, freq, freq_ref=np.inf, P=None):
    """pplib.py:2577-2590."""
    d = Dconst * DM * (freq ** -2.0 - freq_ref ** -2.0)
    return d / P if P else d


def weighted_mean(data, errs=1.0):
    """pplib.py:696-709."""
    if hasattr(errs, "is_integer"):
        errs = np.ones(len(data))
    i = np.where(errs > 0.0)[0]
    w = errs[i] ** -2.0
    return (data[i] * w).sum() / w.sum(), w.sum() ** -0.5


def get_WRMS(data, errs=1.0):
    """The weighted root-mean-square about the weighted mean, weights
    errs**-2 over the points with errs > 0 (pplib.py:711-725)."""
    if hasattr(errs, "is_integer"):
        errs = np.ones(len(data))
    data, errs = np.asarray(data), np.asarray(errs)
    i = np.where(errs > 0.0)[0]
    w_mean = weighted_mean(data, errs)[0]
    w = errs[i] ** -2.0
    return (((data[i] - w_mean) ** 2.0 * w).sum() / w.sum()) ** 0.5


def powlaw(nu, nu_ref, A, alpha):
    """A (nu / nu_ref)**alpha (pplib.py:1048-1052)."""
    return A * (nu / nu_ref) ** alpha


def powlaw_integral(nu2, nu1, nu_ref, A, alpha):
    """The integral of powlaw from nu1 to nu2 (pplib.py:1054-1066)."""
    alpha = np.float64(alpha)
    if alpha == -1.0:
        return A * nu_ref * np.log(nu2 / nu1)
    C = A * (nu_ref ** -alpha) / (1 + alpha)
    return C * (nu2 ** (1 + alpha) - nu1 ** (1 + alpha))


def powlaw_freqs(lo, hi, N, alpha, mid=False):
    """The N + 1 edges between lo and hi of N channels that hold equal flux
    under a power law of index alpha; mid=True returns the N channel centres
    instead (pplib.py:1068-1096)."""
    alpha = np.float64(alpha)
    if alpha == -1.0:
        nus = np.exp(np.linspace(np.log(lo), np.log(hi), N + 1))
    else:
        nus = np.power(np.linspace(lo ** (1 + alpha), hi ** (1 + alpha), N + 1),
                       (1 + alpha) ** -1)
    if mid:
        nus = 0.5 * (nus[:-1] + nus[1:])
    return nus


def fit_powlaw_function(params, freqs, nu_ref, data=None, errs=None):
    """The weighted residuals (data - powlaw) / errs at params = [A, alpha]
    (pplib.py:1204-1217; a plain sequence here, lmfit Parameters there)."""
    A, alpha = params[0], params[1]
    return (data - powlaw(freqs, nu_ref, A, alpha)) / errs


def _chanfit_rows(a, shape):
    """a broadcast to the [nrow, n] of the data."""
    return np.array(np.broadcast_to(np.asarray(a, dtype=np.float64), shape), order="C")


def fit_powlaws(datas, init_params, errs, freqs, nu_refs):
    """fit_powlaw on every row of datas [nrow, n] in one device call
    (ppf_powlaw_fit_rows: Levenberg-Marquardt with leastsq's default ftol and
    xtol, as lmfit's minimize runs it).  errs and freqs are [nrow, n] or [n],
    init_params [2] or [nrow, 2] = amplitude at nu_ref, index, nu_refs a
    scalar or [nrow].  A point whose errs is <= 0, NaN or infinite is left out.
    Returns a DataBunch of arrays over rows: alpha, alpha_err, amp, amp_err,
    cov (of amp and alpha), residuals [nrow, n] = data - model, nu_ref, chi2,
    dof, n_used, status (_lib.CHANFIT_STATUS) and nfev.  A row with fewer than
    3 usable points or a non-finite value at one of them is NaN."""
    datas = np.atleast_2d(np.asarray(datas, dtype=np.float64))
    nrow = datas.shape[0]
    errs = _chanfit_rows(errs, datas.shape)
    freqs = _chanfit_rows(freqs, datas.shape)
    nu_refs = _chanfit_rows(nu_refs, (nrow,))
    init = _chanfit_rows(init_params, (nrow, 2))
    out, info = _engine().powlaw_fit_rows(datas, errs, freqs, nu_refs, init)
    out, info = out.cpu().numpy(), info.cpu().numpy()
    amp, alpha = out[:, 0], out[:, 2]
    with np.errstate(all="ignore"):
        model = powlaw(freqs, nu_refs[:, None], amp[:, None], alpha[:, None])
    return DataBunch(alpha=alpha, alpha_err=out[:, 3], amp=amp, amp_err=out[:, 1], cov=out[:, 4],
                     residuals=datas - model, nu_ref=nu_refs, chi2=out[:, 5], dof=info[:, 2],
                     n_used=info[:, 3], status=info[:, 0], nfev=info[:, 1])


def fit_powlaw(data, init_params, errs, freqs, nu_ref):
    """Fit A (freqs / nu_ref)**alpha to data with uncertainties errs
    (pplib.py:1763-1802): the one-row case of fit_powlaws.  Returns a DataBunch
    with alpha, alpha_err, amp, amp_err, residuals = data - model, nu_ref,
    chi2, dof, and the fit's status and nfev."""
    data = np.asarray(data, dtype=np.float64)
    errs = np.broadcast_to(np.asarray(errs, dtype=np.float64), data.shape)
    r = fit_powlaws(data[None], init_params, errs[None], np.asarray(freqs)[None], nu_ref)
    return DataBunch(alpha=float(r.alpha[0]), alpha_err=float(r.alpha_err[0]),
                     amp=float(r.amp[0]), amp_err=float(r.amp_err[0]), residuals=r.residuals[0],
                     nu_ref=nu_ref, chi2=float(r.chi2[0]), dof=int(r.dof[0]),
                     status=int(r.status[0]), nfev=int(r.nfev[0]))


def fit_DMs_to_freq_resids(freqs, frequency_residuals, errs):
    """fit_DM_to_freq_resids on every row of frequency_residuals [nrow, n] in
    one device call (ppf_line_fit_rows); freqs and errs are [nrow, n] or [n],
    and a point whose errs is <= 0, NaN or infinite is left out.  Returns a
    DataBunch of arrays over rows with fit_DM_to_freq_resids' fields, plus
    n_used and status.  dof = n_used - 2 and chi2 sums the used points."""
    res = np.atleast_2d(np.asarray(frequency_residuals, dtype=np.float64))
    freqs = _chanfit_rows(freqs, res.shape)
    errs = _chanfit_rows(errs, res.shape)
    with np.errstate(all="ignore"):
        used = (errs > 0.0) & np.isfinite(errs)
        x = freqs ** -2
        # the reference hands errs**-2 to polyfit, where 1 / errs would be
        # the usual weight (pplib.py:1819-1820); kept
        w = np.where(used, errs, np.inf) ** -2
        out = _engine().line_fit_rows(x, res, w).cpu().numpy()
        a, b, a_err, b_err, cov = out[:, 0], out[:, 1], out[:, 2] ** 0.5, out[:, 3] ** 0.5, out[:, 4]
        nu_ref = (-b / a) ** -0.5
        nu_ref_err = (((nu_ref ** 2) / 4.0) *
                      (((a_err / a) ** 2) + ((b_err / b) ** 2) - (2 * cov / (a * b)))) ** 0.5
        residuals = res - (a[:, None] * x + b[:, None])
        chi2 = (np.where(used, residuals / np.where(used, errs, 1.0), 0.0) ** 2).sum(axis=1)
        n_used = out[:, 6].astype(np.int64)
        dof = n_used - 2
        chi2 = np.where(np.isnan(a), np.nan, chi2)
        red_chi2 = chi2 / np.where(dof > 0, dof, 1)
    return DataBunch(DM=a / Dconst, DM_err=a_err / Dconst, offset=b, offset_err=b_err,
                     nu_ref=nu_ref, nu_ref_err=nu_ref_err, ab_cov=cov, residuals=residuals,
                     chi2=chi2, dof=dof, red_chi2=red_chi2, n_used=n_used,
                     status=out[:, 7].astype(np.int64))


def fit_DM_to_freq_resids(freqs, frequency_residuals, errs):
    """Fit a DM and a reference frequency to residuals [s] across frequency
    (pplib.py:1804-1840): res = Dconst DM freqs**-2 + offset = Dconst DM
    (freqs**-2 - nu_ref**-2), by a weighted line in freqs**-2 on the device.
    ab_cov is the covariance of the line's two coefficients; nu_ref is NaN
    where -offset / (Dconst DM) < 0."""
    r = fit_DMs_to_freq_resids(np.asarray(freqs)[None], np.asarray(frequency_residuals)[None],
                               np.asarray(errs)[None])
    return DataBunch(DM=float(r.DM[0]), DM_err=float(r.DM_err[0]), offset=float(r.offset[0]),
                     offset_err=float(r.offset_err[0]), nu_ref=float(r.nu_ref[0]),
                     nu_ref_err=float(r.nu_ref_err[0]), ab_cov=float(r.ab_cov[0]),
                     residuals=r.residuals[0], chi2=float(r.chi2[0]), dof=int(r.dof[0]),
                     red_chi2=float(r.red_chi2[0]))


# ---------------------------------------------------------------------------
# GPU-backed utilities (libppfit)
# ---------------------------------------------------------------------------
def get_noise(data, method=None, **kwargs):
    """Estimate the off-pulse noise on the GPU, pplib.py:2206-2225: "PS" from
    the top of the power spectrum (get_noise_PS), "fit" from the power above
    a fitted noise-floor harmonic (get_noise_fit).  method=None takes
    default_noise_method as it is at the call."""
    if method is None:
        method = default_noise_method
    if method == "PS":
        return get_noise_PS(data, **kwargs)
    elif method == "fit":
        return get_noise_fit(data, **kwargs)
    else:
        print("Unknown get_noise method.")
        return 0


def get_noise_PS(data, frac=4, chans=False):
    """Noise from the highest 1/frac of the power spectrum, pplib.py:2227-2253."""
    data = np.asarray(data, dtype=np.float64)
    rows = data if chans else data.ravel()[None]
    out = _engine().noise_rows(rows, frac=frac).cpu().numpy()
    return out if chans else float(out[0])


def get_noise_fit(data, fact=1.1, chans=False):
    """Noise from the power above fact * find_kc(power spectrum), the harmonic
    where a fitted exponential decay meets the noise floor, pplib.py:2255-2287
    (one workgroup per row, ppf_noise_fit_rows)."""
    data = np.asarray(data, dtype=np.float64)
    rows = data if chans else data.ravel()[None]
    out = _engine().noise_fit_rows(rows, fact=fact).cpu().numpy()
    return out if chans else float(out[0])


# host arrays above this many bytes go through _noise_rows in pieces
_NOISE_CHUNK_BYTES = 1 << 28


def _noise_rows(eng, rows):
    """Noise of every row (last axis) by default_noise_method, as a device
    tensor: where the drivers estimate noise_stds and where a fit is asked to
    estimate its own errs."""
    if default_noise_method == "PS":
        fn = eng.noise_rows
    elif default_noise_method == "fit":
        fn = eng.noise_fit_rows
    else:
        raise ValueError("default_noise_method %r is neither 'PS' nor 'fit'"
                         % (default_noise_method,))
    if isinstance(rows, np.ndarray) and rows.ndim > 1 and rows.nbytes > _NOISE_CHUNK_BYTES:
        import torch
        per = max(1, _NOISE_CHUNK_BYTES // max(1, rows[0].nbytes))
        return torch.cat([fn(rows[i:i + per]) for i in range(0, len(rows), per)])
    return fn(rows)


def _fit_errs(eng, data, errs):
    """The errs (or noise) a fit call is given.  None leaves the estimate to
    the fit kernels, which is get_noise_PS per profile; under any other
    default_noise_method it is computed here from the data instead (eng None:
    the default engine, fetched only then)."""
    if errs is not None or default_noise_method == "PS":
        return errs
    if not hasattr(data, "device"):  # not a tensor
        data = np.asarray(data, dtype=np.float64)
    return _noise_rows(eng if eng is not None else _engine(), data)


def half_triangle_function(a, b, dc, N):
    """A half-triangle of base floor(a) and height b on a baseline dc, N long
    (pplib.py:1436-1446)."""
    base = int(np.floor(a))
    out = np.full(int(N), dc, dtype=np.float64)
    k = np.arange(min(base, int(N)))
    out[:len(k)] += np.float64(b) - (np.float64(b) / base) * k  # b at k = 0, 0 at k = base
    return out


def find_kc_function(params, data, errs=1.0, fn="exp_dc"):
    """The (weighted) sum of squares find_kc minimises, pplib.py:1448-1463:
    params = (a, b, dc) of b exp(-a k) + dc ('exp_dc') or of
    half_triangle_function ('half_tri') against data."""
    if fn not in ("exp_dc", "half_tri"):
        return 0.0
    a, b, dc = params[:3]
    n = len(data)
    model = half_triangle_function(a, b, dc, n) if fn == "half_tri" else \
        b * np.exp(-a * np.arange(n)) + dc
    resid = (data - model) / errs
    return np.sum(resid ** 2.0)


def find_kc(pows, errs=1.0, fn="exp_dc"):
    """The harmonic where the noise floor of the power spectrum pows begins,
    pplib.py:1465-1495: the 20 x 20 x 20 grid search of find_kc_function over
    log10(pows) on the device (ppf_find_kc_rows).  errs is a scalar (which
    changes no minimum) or one value per harmonic.  Returns a Python int; an
    unknown fn returns 0.

    Extension: a 2-D pows [nspec, n] returns an int array, one device call
    for all the spectra (errs then applies to each of them)."""
    if fn not in ("exp_dc", "half_tri"):
        return 0
    pows = np.asarray(pows, dtype=np.float64)
    e = None if np.ndim(errs) == 0 else np.asarray(errs, dtype=np.float64)
    kc = _engine().find_kc_rows(pows if pows.ndim > 1 else pows[None], errs=e, fn=fn)[0]
    kc = kc.cpu().numpy()
    return kc.astype(int) if pows.ndim > 1 else int(kc[0])


def get_SNR(prof, fudge=3.25):
    """An estimate of the profile's signal-to-noise ratio from its equivalent
    width (Lorimer & Kramer 2005), pplib.py:2289-2308; the baseline is assumed
    removed."""
    prof = np.asarray(prof, dtype=np.float64)
    area = prof.sum()
    width = area / prof.max()  # equivalent width [bin]
    if width <= 0.0:           # no pulse above the baseline: S/N 0
        return np.float64(0.0) / fudge
    return area / (get_noise(prof) * width ** 0.5) / fudge


def _rot_phases(shape, phase, DM, Ps, freqs, nu_ref):
    """Per-row rotation [rot] implied by rotate_data's arguments (pplib.py:2358-2415)."""
    ndim = len(shape)
    if DM == 0.0:
        nrow = int(np.prod(shape[:-1])) if ndim > 1 else 1
        return np.full(nrow, float(phase))
    d4 = (1,) * (4 - ndim) + tuple(shape)
    nsub, npol, nchan, _ = d4
    D = Dconst * DM / (np.ones(nsub) * Ps)
    f = np.asarray(freqs, dtype=float)
    if f.ndim == 0:
        f = np.ones(nchan) * float(f)
    fterm = (np.tile(f, nsub).reshape(nsub, nchan) if f.ndim == 1 else f) ** -2.0 - \
        nu_ref ** -2.0
    ph = phase + np.array([D[i] * fterm[i] for i in range(nsub)])
    return np.broadcast_to(ph[:, None, :], (nsub, npol, nchan)).ravel()


def rotate_data(data, phase=0.0, DM=0.0, Ps=None, freqs=None, nu_ref=np.inf):
    """Rotate/dedisperse 1-, 2- or 4-D data on the GPU, pplib.py:2338-2426."""
    data = np.asarray(data, dtype=np.float64)
    ph = _rot_phases(data.shape, phase, DM, Ps, freqs, nu_ref)
    rows = data.reshape(-1, data.shape[-1])
    out = _engine().rotate_rows(rows, ph).cpu().numpy()
    if DM == 0.0 or data.ndim in (1, 2, 4):
        return out.reshape(data.shape)
    return out


def rotate_portrait(port, phase=0.0, DM=None, P=None, freqs=None, nu_ref=np.inf):
    """pplib.py:2428-2460."""
    port = np.asarray(port, dtype=np.float64)
    if DM is None and freqs is None:
        ph = np.full(len(port), float(phase))
    else:
        ph = phase + Dconst * DM / P * (np.asarray(freqs) ** -2.0 - nu_ref ** -2.0)
    return _engine().rotate_rows(port, ph).cpu().numpy()


def rotate_profile(profile, phase=0.0):
    """pplib.py:2548-2559."""
    return rotate_data(profile, phase)


def fit_phase_shift(data, model, noise=None, bounds=[-0.5, 0.5], Ns=100):
    """FFTFIT: brute force + Nelder-Mead on the GPU, pplib.py:2054-2100."""
    t0 = time.time()
    noise = _fit_errs(None, data, noise)
    out = _engine().phase_shift_batch(np.asarray(data, dtype=np.float64),
                                      np.asarray(model, dtype=np.float64), noise=noise,
                                      Ns=Ns, bounds=bounds).cpu().numpy()[0]
    return DataBunch(phase=out[0], phase_err=out[1], scale=out[2], scale_err=out[3],
                     snr=out[4], red_chi2=out[5], duration=time.time() - t0)


def normalize_portrait(port, method="rms", weights=None, return_norms=False,
                       get_noise=None):
    """Normalize each profile of a portrait, pplib.py:2462-2507: by its mean,
    its maximum, its fitted scale against the (weighted) mean profile
    ('prof', fit_phase_shift on the device), its noise level ('rms',
    get_noise) or its length ('abs').  All-zero rows stay zero with norm 1."""
    if method not in ("mean", "max", "prof", "rms", "abs"):
        print("Unknown method for normalize_portrait(...), '%s'." % method)
        return None
    noise = get_noise if get_noise is not None else globals()["get_noise"]
    port = np.asarray(port)
    norm_port = np.zeros(port.shape)
    norm_vals = np.ones(len(port))
    if method == "prof":
        good = np.where(port.sum(axis=1) != 0.0)[0]
        w = None if weights is None else np.asarray(weights)[good]
        mean_prof = np.average(port[good], axis=0, weights=w)
    for i in range(len(port)):
        if not port[i].any():
            continue
        if method == "mean":
            nrm = port[i].mean()
        elif method == "max":
            nrm = port[i].max()
        elif method == "prof":
            nrm = fit_phase_shift(port[i], mean_prof).scale
        elif method == "rms":
            nrm = noise(port[i])
        else:
            nrm = (port[i] ** 2).sum() ** 0.5
        norm_port[i] = port[i] / nrm
        norm_vals[i] = nrm
    if return_norms:
        return norm_port, norm_vals
    return norm_port


# ---------------------------------------------------------------------------
# PCA of a portrait and the choice of eigenvectors (ppspline model building)
# ---------------------------------------------------------------------------
def pca(port, mean_prof=None, weights=None, quiet=False, ncomp=None, method=None):
    """Principal components of an nchan x nbin portrait, pplib.py:1497-1534,
    on the device.  method "rows" (ppf_pca_portraits) is a one-sided Jacobi
    on the centred, weighted rows, with no nbin x nbin covariance formed;
    "gram" (ppf_pca_gram_portraits) forms the covariance on the fp64 matrix
    cores and runs the Jacobi on it; None takes "rows" up to 2,048 channels
    and "gram" above (Engine.pca_portraits).

    Returns eigval [r] (descending) and eigvec [nbin, r] (column vectors),
    r = ncomp or min(nchan, nbin): the reference's remaining nbin - r columns
    span the null space of the covariance (their eigenvalues are rounding
    noise) and are not returned; of the r, at most nchan - 1 eigenvalues are
    non-zero.  Each vector's largest-magnitude component is positive
    (LAPACK's sign is arbitrary).  As in the reference, mean_prof does not
    change the covariance (np.cov centres by the weighted mean itself), so
    it is not used.  weights: nchan values >= 0, default equal."""
    port = np.asarray(port, dtype=np.float64)
    nmes, ndim = port.shape
    if not quiet:
        print("Performing principal component analysis on data with %d dimensions and %d "
              "measurements..." % (ndim, nmes))
    if weights is None:
        weights = np.ones(nmes)
    _, eigval, eigvec, _ = _engine().pca_portraits(port, np.asarray(weights, dtype=np.float64),
                                                   ncomp, method)
    return eigval.cpu().numpy(), np.ascontiguousarray(eigvec.cpu().numpy().T)


def reconstruct_portrait(port, mean_prof, eigvec):
    """The portrait projected into the space of the column vectors eigvec
    [nbin, ncomp], pplib.py:1536-1553 (ppf_pca_project)."""
    eigvec = np.asarray(eigvec, dtype=np.float64)
    port = np.asarray(port, dtype=np.float64)
    if eigvec.shape[1] == 0:
        return np.tile(np.asarray(mean_prof, dtype=np.float64), (len(port), 1))
    return _engine().pca_project(port, mean_prof, np.ascontiguousarray(eigvec.T),
                                 reconstruct=True)[1].cpu().numpy()


def count_crossings(x, x0):
    """Number of crossings of the 1-D array x across the threshold x0,
    pplib.py:686-694 (an exact hit counts once, not twice)."""
    d = np.asarray(x) - x0
    return (np.diff(np.sign(d)) != 0).sum() - (d == 0).sum()


_NO_SMOOTH = ("wavelet smoothing is unpinned: PyWavelets is not available to pin it against "
              "(only try_nlevels=0, the identity, is implemented)")


def _check_wavelet(wavelet):
    if wavelet != "db8":
        raise NotImplementedError("wavelet %r: only 'db8' is built" % (wavelet,))


def wavelet_smooth(port, wavelet="db8", nlevel=5, threshtype="hard", fact=1.0):
    """The wavelet-denoised portrait [nchan, nbin] or profile [nbin],
    pplib.py:1621-1666, on the device (ppf_wavelet_smooth_rows): the
    undecimated db8 transform with periodic extension to nlevel levels, the
    threshold fact median(|a_L u d_L|) / 0.6745 sqrt(2 ln nbin) on every
    coefficient array ('hard' or 'soft'), and the inverse.  Built from the
    transform's definition and not pinned against PyWavelets (DESIGN.md
    section 9).  nbin must be a multiple of 2^nlevel (ValueError, as
    pywt.swt)."""
    _check_wavelet(wavelet)
    if threshtype not in ("hard", "soft"):
        raise ValueError("threshtype %r: 'hard' or 'soft'" % (threshtype,))
    port = np.asarray(port, dtype=np.float64)
    nbin, nlevel = port.shape[-1], int(nlevel)
    if nlevel < 1 or nbin % (1 << nlevel):
        raise ValueError("nlevel=%d: the length of the data, %d, must be a multiple of 2^nlevel"
                         % (nlevel, nbin))
    return _engine().wavelet_smooth_rows(port, nlevel, float(fact), threshtype).cpu().numpy()


def get_red_chi2(data, model, errs=None, dof=None):
    """Reduced chi-squared of 1- or 2-D data against model, pplib.py:727-750:
    errs default to get_noise of the data (per row), dof to sum(data.shape)."""
    data, model = np.asarray(data, dtype=np.float64), np.asarray(model, dtype=np.float64)
    resids = data - model
    if errs is None:
        errs = get_noise(data, chans=data.ndim == 2)
    if dof is None:
        dof = sum(data.shape)
    if data.ndim == 1:
        return np.sum((resids / errs) ** 2.0) / dof
    return np.array([(resids[ii] / np.asarray(errs)[ii]) ** 2.0
                     for ii in range(len(resids))]).sum() / dof


def fit_wavelet_smooth_function(fact, prof, wavelet, nlevel, threshtype, rchi2_tol):
    """The negative pseudo-S/N of the profile smoothed at (nlevel, fact) that
    smart_smooth minimises, pplib.py:1737-1761 (ppf_wavelet_objective_rows):
    0 when the smoothed profile's reduced chi-squared is further than
    rchi2_tol from 1."""
    _check_wavelet(wavelet)
    obj, _ = _engine().wavelet_objective_rows(np.asarray(prof, dtype=np.float64), int(nlevel),
                                              float(np.ravel(fact)[0]), threshtype, rchi2_tol)
    return float(obj.cpu().numpy())


def smart_smooth_levels(nbin, try_nlevels=None):
    """The number of levels smart_smooth searches for profiles of nbin bins
    (pplib.py:1688-1701): 0 (the input is returned) for try_nlevels=0 or an
    odd nbin, 1 for an nbin that is no power of two, else try_nlevels or its
    default log2(nbin)."""
    if try_nlevels == 0 or nbin % 2 != 0:
        return 0
    if nbin & (nbin - 1):
        return 1
    return int(np.log2(nbin)) if try_nlevels is None else int(try_nlevels)


def smart_smooth(port, try_nlevels=None, rchi2_tol=0.1, full=False, **kwargs):
    """wavelet_smooth at the (nlevel, fact) of largest pseudo-S/N per profile,
    pplib.py:1668-1735, every profile of port [nchan, nbin] (or one [nbin])
    in one device call (ppf_smart_smooth_rows): per level 1 .. try_nlevels the
    reference's opt.brute over fact (30 grid points on [0, 3], then fmin), the
    first level of least objective, and zeros when the result's reduced
    chi-squared is further than rchi2_tol from 1.  kwargs: threshtype is
    used, nlevel and fact are dropped, wavelet must be 'db8'.  full=True
    (not in the reference) returns a dict with the search's results too:
    smooth, nlevel, fact, red_chi2, zeroed and fun_vals [..., try_nlevels]."""
    _check_wavelet(kwargs.get("wavelet", "db8"))
    threshtype = kwargs.get("threshtype", "hard")
    if threshtype not in ("hard", "soft"):
        raise ValueError("threshtype %r: 'hard' or 'soft'" % (threshtype,))
    port_in = port
    port = np.asarray(port, dtype=np.float64)
    L = smart_smooth_levels(port.shape[-1], try_nlevels)
    if L == 0:
        if not full:
            return port_in
        lead = port.shape[:-1]
        return dict(smooth=port, nlevel=np.zeros(lead, dtype=int), fact=np.zeros(lead),
                    red_chi2=np.zeros(lead), zeroed=np.zeros(lead, dtype=bool), fun_vals=None)
    out = _engine().smart_smooth_rows(port, L, rchi2_tol, threshtype, table=full)
    smooth = out[0].cpu().numpy()
    if not full:
        return smooth
    return dict(smooth=smooth, nlevel=out[1].cpu().numpy().astype(int), fact=out[2].cpu().numpy(),
                red_chi2=out[3].cpu().numpy(), zeroed=out[4].cpu().numpy().astype(bool),
                fun_vals=out[5].cpu().numpy())


def find_significant_eigvec(eigvec, check_max=10, return_max=10, snr_cutoff=150.0,
                            check_crossings=True, check_acorr=True, return_smooth=False,
                            noise=None, smooth=False, smooth_eigvec=None, **kwargs):
    """Indices of the "significant" eigenvectors (columns of eigvec
    [nbin, ncomp]), pplib.py:1555-1619, with the reference's control flow --
    its borderline `elif`, which can never add a vector, included.

    smooth=False (the default): the smoothing is the identity (the
    reference's try_nlevels=0 path of smart_smooth); return_smooth=True or
    another try_nlevels raises NotImplementedError, and other smart_smooth
    keywords (rchi2_tol, ...) are accepted and unused.

    smooth="swt": every vector that may be examined goes through smart_smooth
    (**kwargs: try_nlevels, rchi2_tol, threshtype) in one device call up
    front, and the S/N test takes the smoothed vector with the noise of the
    unsmoothed one, as in the reference; return_smooth=True then returns
    (ieig, smooth_eigvec [nbin, ncomp], zero but for the columns ieig).
    smooth_eigvec: those smoothed vectors [nbin, >= ncheck] if already known.

    noise: the vectors' get_noise values if already known (default:
    get_noise of the examined vectors, on the device)."""
    if smooth not in (False, None, "swt"):
        raise NotImplementedError(_NO_SMOOTH)
    swt = smooth == "swt"
    if not swt and (return_smooth or kwargs.get("try_nlevels", 0) not in (0, None)):
        raise NotImplementedError(_NO_SMOOTH)
    eigvec = np.asarray(eigvec, dtype=np.float64)
    ncheck = min(max(check_max, return_max), eigvec.shape[1])
    if noise is None and ncheck:
        noise = get_noise(np.ascontiguousarray(eigvec.T[:ncheck]), chans=True)
    evs = eigvec.T
    if swt and ncheck:
        if smooth_eigvec is None:
            evs = smart_smooth(np.ascontiguousarray(eigvec.T[:ncheck]), **kwargs)
        else:
            evs = np.asarray(smooth_eigvec, dtype=np.float64).T
    smooth_out = np.zeros(eigvec.shape)
    ieig = []
    for ivec in range(ncheck):  # (the reference always has nbin columns)
        add_eigvec = False
        ev = evs[ivec]
        ev_noise = noise[ivec] * np.sqrt(len(ev) / 2.0)
        ev_snr = np.sum(np.abs(np.fft.rfft(ev)[1:]) ** 2) / ev_noise
        if ev_snr >= snr_cutoff:
            if check_crossings and ev_snr < 3 * snr_cutoff:
                ncross = count_crossings(abs(ev), 0.1 * abs(ev).max())
                if ncross < int(0.02 * len(ev)):
                    add_eigvec = True
            elif check_acorr and ev_snr < 3 * snr_cutoff and add_eigvec:
                acorr = np.correlate(ev, ev, "same")
                fwhm = acorr.argmax() - np.where(acorr > acorr.max() / 2.0)[0].min()
                if fwhm > 5:
                    add_eigvec = True
                else:
                    add_eigvec = False
                    print("Borderline case eigenvector %d failed test." % ivec)
            else:
                add_eigvec = True
        if add_eigvec:
            ieig.append(ivec)
            smooth_out[:, ivec] = ev
        if ivec + 1 == check_max:
            break
        if len(ieig) == return_max:
            break
    if return_smooth:
        return np.array(ieig, dtype=int), smooth_out
    return np.array(ieig, dtype=int)


def fit_portrait(data, model, init_params, P, freqs, nu_fit=None, nu_out=None, errs=None,
                 bounds=[(None, None), (None, None)], id=None, quiet=True):
    """Legacy phase + DM fit (pplib.py:2102-2204) on the GPU.

    As the reference, scipy TNC (jac, bounds, xtol 1e-10; pplib.py:2144-2148)
    over (phase, DM) -- the device TNC (ppfit_tnc.hip) in its 2-parameter
    form -- then the legacy outputs: phase/DM errors from the 2x2 curvature
    matrix without amplitude covariance (pplib.py:2184-2190) and scale_errs
    = (p_n / errs^2)^-1/2 (pplib.py:2197).  return_code and nfeval are TNC's
    (RCSTRINGS, pplib.py:111-119).
    """
    from . import pptoaslib
    freqs = np.asarray(freqs, dtype=float)
    if nu_fit is None:
        nu_fit = freqs.mean()
    b = list(bounds) if bounds is not None else [(None, None)] * 2
    res = pptoaslib._fit_batch_host(
        np.asarray(data, float)[None], np.asarray(model, float)[None], [init_params[0],
        init_params[1], 0.0, 0.0, 0.0], P, freqs, [nu_fit, nu_fit, nu_fit],
        [nu_out, nu_out, nu_out], errs, [1, 1, 0, 0, 0], log10_tau=False, legacy=True,
        method="TNC-legacy", bounds=b + [(None, None)] * 3)
    r = {k: v[0] for k, v in res.items() if k != "legacy"}
    leg = {k: v[0] for k, v in res["legacy"].items()}
    return DataBunch(phase=r["params"][0], phase_err=leg["phase_err"], DM=r["params"][1],
                     DM_err=leg["DM_err"], scales=r["scales"], scale_errs=leg["scale_errs"],
                     nu_ref=r["nu_out"][0], covariance=leg["covariance"], chi2=r["chi2"],
                     red_chi2=r["red_chi2"], snr=r["snr"], duration=r["duration"],
                     nfeval=int(r["nfev"]), return_code=int(r["status"]))


# ---------------------------------------------------------------------------
# Fake data and archive output (pplib.py:1146-1174, 2509-2546, 3039-3384):
# PSRFITS files written by psrfits.PSRFITSWriter from 16-bit samples that
# the device packs (ppf_pack_subints) or generates (ppf_fake_subints)
# ---------------------------------------------------------------------------
def _scint_pattern(nchan, params=None, nsin=2, amax=1.0, wmax=3.0, rng=None):
    """add_scintillation's per-channel pattern (pplib.py:1159-1173); rng: a
    numpy Generator for the random parameters (None: numpy's global state)."""
    rng = np.random if rng is None else rng
    if params is None:
        params = []
        for _ in range(nsin):
            params += [rng.uniform(0, amax), rng.chisquare(wmax), rng.uniform(0, 1)]
    pattern = np.zeros(nchan)
    for isin in range(len(params) // 3):
        a, w, p = params[isin * 3:isin * 3 + 3]
        pattern += a * np.sin(np.linspace(0, w * np.pi, nchan) + p * np.pi) ** 2
    return pattern


def add_scintillation(port, params=None, random=True, nsin=2, amax=1.0, wmax=3.0, rng=None):
    """pplib.py:1146-1174 (host numpy); rng: see _scint_pattern."""
    port = np.asarray(port, dtype=np.float64)
    if params is None and random is False:
        return port
    return port * _scint_pattern(len(port), params, nsin, amax, wmax, rng)[:, None]


def _DM_nu_term(freqs, xs, Cs, nu_ref):
    """add_DM_nu's frequency term sum_i C_i (nu**x_i - nu_ref**x_i), pplib.py:2536-2542."""
    if not hasattr(Cs, "__iter__"):
        Cs = np.ones(len(xs))
    Cs = list(Cs) + [1.0] * (len(xs) - len(Cs))
    freqs = np.asarray(freqs, dtype=np.float64)
    term = np.zeros(freqs.shape)
    for C, x in zip(Cs, xs):
        term = term + C * (freqs ** x - nu_ref ** x)
    return term


def add_DM_nu(port, phase=0.0, DM=None, P=None, freqs=None, xs=[-2.0], Cs=[1.0], nu_ref=np.inf):
    """pplib.py:2509-2546 (host numpy)."""
    port = np.asarray(port, dtype=np.float64)
    pFFT = np.fft.rfft(port, axis=1)
    k = np.arange(pFFT.shape[1])
    if DM is None and freqs is None:
        rot = np.full(len(port), float(phase))
    else:
        rot = phase + Dconst * DM / P * _DM_nu_term(freqs, xs, Cs, nu_ref)
    return np.fft.irfft(pFFT * np.exp(2.0j * np.pi * rot[:, None] * k), port.shape[1], axis=1)


def read_ephemeris(ephemeris):
    """The fields write_archive and make_fake_pulsar take from a parameter
    file, by the reference's own parse (pplib.py:3133-3147, 3284-3302): PSR
    or PSRJ, RAJ, DECJ, DM, F0 or P0, PEPOCH; plus the file's text."""
    with open(ephemeris, "r") as fh:
        text = fh.read()
    par = DataBunch(PSR="noname", RAJ="00:00:00.0", DECJ="+00:00:00.0", DM=0.0, P0=None,
                    PEPOCH=None, text=text)
    for line in text.splitlines():
        f = line.split()
        if len(f) < 2:
            continue
        if f[0] in ("PSR", "PSRJ"):
            par.PSR = f[1]
        elif f[0] in ("RAJ", "DECJ"):
            par[f[0]] = f[1]
        elif f[0] == "F0":
            par.P0 = np.float64(f[1].replace("D", "E")) ** -1
        elif f[0] in ("P0", "PEPOCH", "DM"):
            par[f[0]] = np.float64(f[1].replace("D", "E"))
    if par.DECJ[0] not in "+-":
        par.DECJ = "+" + par.DECJ
    return par


def _as_MJD(x, default):
    from .mjd import MJD
    if x is None:
        x = default
    return x if isinstance(x, MJD) else MJD(x)


def _chunk_subints(eng, npol, nchan, nbin):
    """Subints per chunk of an archive being written: a chunk's fp64 rows and
    int16 samples within the engine's workspace limit, and at most 1 GiB so
    that the host writes one chunk while the device makes the next."""
    budget = min(eng.workspace_limit(), 1 << 30)
    return max(1, budget // (10 * npol * nchan * nbin))


def _write_chunks(w, nsub, chunk, make, freqs, weights, tsubint, offs_sub, period, par_ang):
    """make(lo, hi) -> device (raw, scl, offs) of subints lo:hi, appended to
    the writer w; the previous chunk is written (a thread in the C writer)
    while the device makes this one."""
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(1) as pool:
        pending = None
        for lo in range(0, nsub, chunk):
            hi = min(nsub, lo + chunk)
            raw, scl, offs = (t.cpu().numpy() for t in make(lo, hi))
            if pending is not None:
                pending.result()
            pending = pool.submit(w.write, raw, scl, offs, freqs[lo:hi], weights[lo:hi],
                                  tsubint[lo:hi], offs_sub[lo:hi], period[lo:hi], par_ang[lo:hi])
        if pending is not None:
            pending.result()


def _unload(outfile, data, meta, rot=None):
    """Write data [nsub, npol, nchan, nbin] (host array or device tensor) as a
    PSRFITS file: per chunk, optionally rotated by rot [nsub, nchan] [rot],
    packed on the device and appended.  meta: PSRFITSWriter's keywords plus
    freqs, weights [nsub, nchan] and tsubint, offs_sub, period, par_ang [nsub]."""
    import torch
    from .psrfits import PSRFITSWriter
    eng = _engine()
    nsub, npol, nchan, nbin = tuple(data.shape)
    meta = dict(meta)
    rows = [np.asarray(meta.pop(k), dtype=np.float64) for k in
            ("freqs", "weights", "tsubint", "offs_sub", "period", "par_ang")]

    def make(lo, hi):
        d = data[lo:hi]
        if isinstance(d, torch.Tensor):
            d = d.to(device=eng.device, dtype=torch.float64).contiguous()
            if rot is not None and d.data_ptr() == data[lo:hi].data_ptr():
                d = d.clone()  # the caller's tensor is not rotated
        else:
            d = torch.as_tensor(np.ascontiguousarray(d, dtype=np.float64), device=eng.device)
        if rot is not None:
            eng.rotate_rows(d, np.repeat(rot[lo:hi, None, :], npol, axis=1), inplace=True)
        return eng.pack_subints(d)

    with PSRFITSWriter(outfile, npol, nchan, nbin, **meta) as w:
        _write_chunks(w, nsub, _chunk_subints(eng, npol, nchan, nbin), make, *rows)


def write_archive(data, ephemeris, freqs, nu0=None, bw=None, outfile="pparchive.fits", tsub=1.0,
                  start_MJD=None, weights=None, dedispersed=False, state="Stokes",
                  telescope="GBT", quiet=False):
    """pplib.py:3077-3187 without PSRCHIVE: a fold-mode PSRFITS file written
    by the package (psrfits.PSRFITSWriter, 16-bit samples packed on the
    device).  data [nsub, npol, nchan, nbin], a host array or a device
    tensor, is taken dedispersed; with dedispersed=False it is stored
    rotated to the dispersed state by the ephemeris DM about nu0, the
    rotation load_data(..., dedisperse=True) undoes
    (archive.dedispersion_phases).  The ephemeris parse is read_ephemeris;
    the period (1 / F0 or P0) is constant and goes into the PERIOD column,
    there are no polycos.  Epochs are start_MJD + tsub / 2 + i tsub;
    start_MJD is an mjd.MJD or a float [day] (None: MJD 50000)."""
    from .archive import dedispersion_phases
    nsub, npol, nchan, nbin = tuple(data.shape)
    freqs = np.asarray(freqs, dtype=np.float64)
    if nu0 is None:
        nu0 = freqs.mean()
    if bw is None:
        bw = (freqs.max() - freqs.min()) + abs(freqs[1] - freqs[0])
    par = read_ephemeris(ephemeris)
    if par.P0 is None:
        raise ValueError("%s has neither F0 nor P0" % ephemeris)
    Ps = np.full(nsub, float(par.P0))
    fr = np.tile(freqs, (nsub, 1))
    rot = None if dedispersed else -dedispersion_phases(fr, Ps, float(par.DM), float(nu0))
    meta = dict(start=_as_MJD(start_MJD, 50000.0), nu0=nu0, bw=bw, DM=par.DM,
                dedispersed=dedispersed, state=state, telescope=telescope, source=par.PSR,
                ra=par.RAJ, dec=par.DECJ, ephemeris=par.text, freqs=fr,
                weights=np.ones((nsub, nchan)) if weights is None else weights,
                tsubint=np.full(nsub, float(tsub)), offs_sub=tsub / 2.0 + tsub * np.arange(nsub),
                period=Ps, par_ang=np.zeros(nsub))
    _unload(outfile, data, meta, rot)
    if not quiet:
        print("\nUnloaded %s.\n" % outfile)


def unload_new_archive(data, arch, outfile, DM=None, dmc=0, weights=None, quiet=False):
    """pplib.py:3039-3075 without PSRCHIVE: data [nsub, npol, nchan, nbin]
    (host array or device tensor, in the state dmc says) written as a PSRFITS
    file with the metadata of arch -- a load_data bunch, or the name of an
    archive load_data reads.  DM and weights replace arch's when given.
    Epochs are stored as offsets from the first epoch's whole second."""
    from . import archive as _archive
    if isinstance(arch, str):
        arch = _archive.open_archive(arch, rm_baseline=False).meta
    b = _archive.normalize(arch, str(outfile), subints="subints" in arch)
    nsub, npol, nchan, nbin = tuple(data.shape)
    if (nsub, nchan, nbin) != (b.nsub, b.nchan, b.nbin):
        raise ValueError("data %s does not fit the archive (%d, npol, %d, %d)" % (
            tuple(data.shape), b.nsub, b.nchan, b.nbin))
    e0 = b.epochs[0]
    offs_sub = np.array([(e.days - e0.days) * 86400.0 + (e.secs - e0.secs) + e.fracsec
                         for e in b.epochs])
    from .mjd import MJD
    meta = dict(start=MJD(e0.days, e0.secs, 0.0), nu0=b.nu0, bw=b.bw,
                DM=b.DM if DM is None else DM, dedispersed=bool(dmc), state=b.state,
                telescope=b.telescope, frontend=b.frontend, backend=b.backend,
                backend_delay=b.backend_delay, source=b.source, freqs=b.freqs,
                weights=b.weights if weights is None else weights, tsubint=b.subtimes,
                offs_sub=offs_sub, period=b.Ps, par_ang=b.parallactic_angles)
    _unload(outfile, data, meta)
    if not quiet:
        print("\nUnloaded %s.\n" % outfile)


def scrunch_archive(datafile, outfile, nchan=None, nbin=None, tscrunch=False, quiet=False):
    """Write datafile at lower resolution as the PSRFITS file outfile: the
    stand-in for `pam --setnchn nchan --setnbin nbin [-T] -e ...`, not pinned
    against pam.  The data are read as stored (no baseline removed),
    scrunched by archive.scrunch -- see there for the group frequencies,
    weights and phases and for the bin-centre offset of the bscrunch -- and
    written by unload_new_archive with the scrunched frequencies and weights,
    in the dedispersion state the input is stored in.  Returns outfile."""
    from . import archive as _archive
    b = _archive.scrunch(datafile, nchan=nchan, nbin=nbin, tscrunch=tscrunch, rm_baseline=False)
    unload_new_archive(b.subints, b, outfile, DM=b.DM, dmc=int(b.dmc), quiet=quiet)
    return outfile


def scrunched_profile(bunch):
    """The T-, P- and F-scrunched profile [nbin] of a load_data bunch loaded as
    stored (pscrunch=True; subints on the host or the device): per subint the
    dedispersed, weighted sum over channels (Engine.rotate_fscrunch with the
    rotation load_data(dedisperse=True) applies, none when the archive is
    stored dedispersed, and the archive's weights), the subints added and
    divided by the sum of every weight -- arch.tscrunch() then arch.fscrunch()
    with PSRCHIVE's weighted means.  Zeros when no weight is positive."""
    from .archive import stored_dedispersion_phases
    w = np.asarray(bunch.weights, dtype=np.float64)
    profs = _engine().rotate_fscrunch(bunch.subints[:, 0], stored_dedispersion_phases(bunch), w)
    wsum = w.sum()
    prof = profs.sum(dim=0).cpu().numpy()
    return prof / wsum if wsum > 0.0 else np.zeros_like(prof)


def make_constant_portrait(archive, outfile, profile=None, DM=0.0, dmc=False, weights=None,
                           quiet=False):
    """Fill an archive with one profile, pplib.py:958-994 without PSRCHIVE:
    outfile gets the nsub, npol, nchan, nbin, frequencies, epochs, etc. of
    archive (an archive load_data reads) and profile [nbin] in every (subint,
    polarisation, channel), stored with header DM ``DM`` in the state ``dmc``
    says, with ``weights`` [nsub, nchan] (ones when None), through
    unload_new_archive.  profile=None: the archive's own T-, P- and F-scrunched
    profile (scrunched_profile).  A profile whose length is not the archive's
    nbin is a ValueError (an assertion in the reference)."""
    from . import archive as _archive
    meta = _archive.open_archive(archive, rm_baseline=False).meta
    if profile is None:
        profile = scrunched_profile(_archive.load_data(
            archive, dedisperse=False, tscrunch=False, pscrunch=True, rm_baseline=False,
            quiet=True, host=False))
    profile = np.asarray(profile, dtype=np.float64)
    nsub, npol, nchan, nbin = meta.nsub, meta.npol, meta.nchan, meta.nbin
    if profile.ndim != 1 or len(profile) != nbin:
        raise ValueError("len(profile) != number of bins in dummy archive (%s, %d)" % (
            profile.shape, nbin))
    if weights is None:
        weights = np.ones([nsub, nchan])
    data = np.empty([nsub, npol, nchan, nbin])
    data[...] = profile
    unload_new_archive(data, meta, outfile, DM=DM, dmc=dmc, weights=weights, quiet=quiet)


def make_fake_pulsar(modelfile, ephemeris, outfile="fake_pulsar.fits", nsub=1, npol=1, nchan=512,
                     nbin=2048, nu0=1500.0, bw=800.0, tsub=300.0, phase=0.0, dDM=0.0,
                     start_MJD=None, weights=None, noise_stds=1.0, scales=1.0, dedispersed=False,
                     t_scat=0.0, alpha=scattering_alpha, scint=False, xs=None, Cs=None,
                     nu_DM=np.inf, state="Stokes", telescope="GBT", quiet=False, seed=None):
    """pplib.py:3189-3384 without PSRCHIVE: fake pulsar data generated on
    the device (ppf_fake_subints: the model rows of read_model_device, one
    rotation, amplitude and Philox noise stream per profile, quantised to
    16-bit samples as they are made) and written as a PSRFITS file in chunks.
    Arguments are the reference's; the folding period is the ephemeris's
    constant 1 / F0 (or P0), and every polarisation holds the same model with
    its own noise.  seed (None: fresh entropy) fixes the noise and, with
    scint=True, the scintillation pattern drawn per subint from a
    numpy.random.Generator.

    Two deliberate deviations from the reference's HEAD:
    - phase and dDM act when xs is None too, as rotate_data(model, -phase,
      -dDM, P, freqs, nu0); the reference ignores them there
      (pplib.py:3347-3349), against its own docstring;
    - phase and dDM may each be an array of length nsub (one per subint).
    """
    from .archive import dedispersion_phases
    chanwidth = bw / nchan
    lofreq = nu0 - (bw / 2)
    freqs = np.linspace(lofreq + (chanwidth / 2.0), lofreq + bw - (chanwidth / 2.0), nchan)
    noise_stds = np.asarray(noise_stds, dtype=np.float64)
    if noise_stds.ndim and len(noise_stds) != nchan:
        print("\nlen(noise_stds) != nchan\n")
        return 0
    scales = np.asarray(scales, dtype=np.float64)
    if scales.ndim and len(scales) != nchan:
        print("\nlen(scales) != nchan\n")
        return 0
    par = read_ephemeris(ephemeris)
    if par.P0 is None:
        raise ValueError("%s has neither F0 nor P0" % ephemeris)
    P, DM = float(par.P0), float(par.DM)
    start = _as_MJD(start_MJD, par.PEPOCH if par.PEPOCH is not None else 50000.0)
    tau_model = read_model(modelfile, quiet=True)[4][1]
    name, ngauss, model = read_model_device(modelfile, nbin, freqs, P, quiet=True)
    if t_scat and not tau_model:  # modelfile overrides
        taus = scattering_times(t_scat / P, alpha, freqs, nu0)
        model = _engine().scatter_rotate_rows(model, 0.0, taus)
    # every rotation of a profile in one phase [rot]
    ph = np.ones(nsub) * phase
    dDMs = np.ones(nsub) * dDM
    if xs is None:
        term = freqs ** -2.0 - nu0 ** -2.0
    else:
        ph = phase_transform(ph, DM + dDMs, nu0, nu_DM, P)
        term = _DM_nu_term(freqs, xs, Cs, nu_DM)
    rot = -ph[:, None] - (Dconst * dDMs / P)[:, None] * term[None, :]
    Ps = np.full(nsub, P)
    fr = np.tile(freqs, (nsub, 1))
    if not dedispersed:
        rot = rot - dedispersion_phases(fr, Ps, DM, nu0)
    rng = np.random.default_rng(seed)
    amp = np.ones((nsub, nchan)) * scales
    if scint is not False:
        for isub in range(nsub):
            amp[isub] *= _scint_pattern(nchan, nsin=3, amax=1.0, wmax=5.0, rng=rng) \
                if scint is True else _scint_pattern(nchan, scint)
    noise_seed = int(rng.integers(0, 2 ** 63)) if seed is None else int(seed)
    eng = _engine()

    def make(lo, hi):
        return eng.fake_subints(model, rot[lo:hi], amp[lo:hi], noise_stds, noise_seed, sub0=lo,
                                npol=npol, packed=True)

    from .psrfits import PSRFITSWriter
    with PSRFITSWriter(outfile, npol, nchan, nbin, start, nu0, bw, DM=DM,
                       dedispersed=dedispersed, state=state, telescope=telescope,
                       source=par.PSR, ra=par.RAJ, dec=par.DECJ, ephemeris=par.text) as w:
        _write_chunks(w, nsub, _chunk_subints(eng, npol, nchan, nbin), make, fr,
                      np.ones((nsub, nchan)) if weights is None else np.asarray(weights, float),
                      np.full(nsub, float(tsub)), tsub / 2.0 + tsub * np.arange(nsub), Ps,
                      np.zeros(nsub))
    if not quiet:
        print("\nUnloaded %s.\n" % outfile)


# ---------------------------------------------------------------------------
# TOA output (pplib.py:3386-3509)
# ---------------------------------------------------------------------------
def filter_TOAs(TOAs, flag, cutoff, criterion=">=", pass_unflagged=False,
                return_culled=False):
    """pplib.py:3386-3413."""
    import operator
    op = {">=": operator.ge, ">": operator.gt, "<=": operator.le, "<": operator.lt,
          "==": operator.eq, "!=": operator.ne}[criterion]
    keep, cull = [], []
    for toa in TOAs:
        if hasattr(toa, flag):
            (keep if op(getattr(toa, flag), cutoff) else cull).append(toa)
        elif pass_unflagged:
            keep.append(toa)
        else:
            cull.append(toa)
    if return_culled:
        return keep, return_culled
    return keep


def _flag_fmt(flag, vtype):
    """Format of one flag in write_TOAs' Python-2 formatting (pplib.py:3486-3503)
    for a value of type vtype: str %s, int %d, '_cov' %.1e, 'phs' %.8f, 'flux'
    %.5f, else %.3f."""
    f = flag.replace("%", "%%")
    if hasattr(vtype, "lower"):
        return " -%s %%s" % f
    # Python-2 ints -- bool included (True.bit_length() exists, so
    # pptoas.py:1602's DM_mean=True prints "1") -- take %d; numpy's bool_ has
    # no bit_length and takes the float formats
    if issubclass(vtype, (int, np.integer)) and not issubclass(vtype, np.bool_):
        return " -%s %%d" % f
    if flag.find("_cov") >= 0:
        return " -%s %%.1e" % f
    if flag.find("phs") >= 0:
        return " -%s %%.8f" % f
    if flag.find("flux") >= 0:
        return " -%s %%.5f" % f
    return " -%s %%.3f" % f


def _flag_text(flag, value):
    """One flag as write_TOAs prints it (pplib.py:3486-3503)."""
    return _flag_fmt(flag, type(value)) % value


_LINE_FMTS = {}  # (flag names, value types) of a TOA's flags -> their joined format
_NoneType = type(None)


def toa_line(toa, inf_is_zero=True):
    """One loosely-IPTA .tim line, pplib.py:3471-3503.  The flags of every TOA
    with the same (flag, value type) signature share one format string; a
    None value is left out, as write_TOAs skips it."""
    freq = 0.0 if (toa.frequency == np.inf and inf_is_zero) else toa.frequency
    m = toa.MJD
    s = "%s %.8f %d" % (toa.archive, freq, m.intday()) + \
        ("%.15f   %.3f  %s" % (m.fracday(), toa.TOA_error, toa.telescope_code))[1:]
    if toa.DM is not None:
        s += " -pp_dm %.7f" % toa.DM
    if toa.DM_error is not None:
        s += " -pp_dme %.7f" % toa.DM_error
    fl = toa.flags
    vals = tuple(fl.values())
    types = tuple(map(type, vals))
    key = (tuple(fl), types)
    fmt = _LINE_FMTS.get(key)
    if fmt is None:
        fmt = "".join([_flag_fmt(k, t) for k, t in zip(key[0], types) if t is not _NoneType])
        if len(_LINE_FMTS) < 4096:
            _LINE_FMTS[key] = fmt
    if _NoneType in types:
        vals = tuple([v for v in vals if v is not None])
    return s + fmt % vals


def write_TOAs(TOAs, inf_is_zero=True, SNR_cutoff=0.0, outfile=None, append=True):
    """pplib.py:3451-3509.  A get_TOAs TOA_list (toas.TOAList) is written
    through its column blocks (native .tim writer, include/pptim.h, straight
    from its buffers to the file); any other sequence of TOAs one line at a
    time.  Returns None, as the reference does."""
    from .toas import TOAList, write_pieces
    if isinstance(TOAs, TOAList):
        pieces = TOAs.tim_chunks(inf_is_zero, SNR_cutoff)
        if outfile is None:
            sys.stdout.flush()
            write_pieces(sys.stdout.buffer, pieces)
            sys.stdout.buffer.flush()
        else:
            with open(outfile, "ab" if append else "wb") as f:
                write_pieces(f, pieces)
        return None
    toas = TOAs if hasattr(TOAs, "__len__") else [TOAs]
    toas = filter_TOAs(toas, "snr", SNR_cutoff, ">=", pass_unflagged=False)
    lines = [toa_line(t, inf_is_zero) for t in toas]
    if outfile is None:
        for ln in lines:
            print(ln)
    else:
        with open(outfile, "a" if append else "w") as f:
            for ln in lines:
                f.write(ln + "\n")
