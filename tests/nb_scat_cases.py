"""Shared by the narrowband phase + tau tests (CPU and GPU): the fixture's
cases and the oracle's per-channel fit.

One channel's fit is oracle.ppfit_oracle.fit_portrait_full on a one-channel
portrait with fit_flags [1, 0, 0, 1, 0] and nu_fits = nu_outs = the channel's
frequency (tests/golden/make_golden_nb_scat.py runs the reference the same
way).
"""
import functools
import os

import numpy as np

from oracle import ppfit_oracle as O

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MAIN = "nb_scat.npz"     # make_golden_nb_scat.py: even lengths
ODD = "nb_scat_odd.npz"  # make_golden_nb_scat_odd.py: nbin 999 and 2049
FLAGS = [1, 0, 0, 1, 0]
OUT_KEYS = ["phi", "phi_err", "tau", "tau_err", "scale", "scale_err", "snr", "red_chi2"]


@functools.lru_cache(maxsize=None)
def fixture(name=MAIN):
    return np.load(os.path.join(GOLDEN_DIR, name), allow_pickle=False)


def case(ic, name=MAIN):
    g = fixture(name)
    k = "c%d_" % ic
    c = {name[len(k):]: g[name] for name in g.files if name.startswith(k)}
    c["nbin"], c["log10"] = int(c["nbin"]), bool(c["log10"])
    c["P"] = float(g["P"])
    return c


def ncase(name=MAIN):
    return int(fixture(name)["ncase"])


def scattered_cases(name=MAIN):
    return [i for i in range(ncase(name)) if float(case(i, name)["tau_inj"]) != 0.0]


def unscattered_cases(name=MAIN):
    return [i for i in range(ncase(name)) if float(case(i, name)["tau_inj"]) == 0.0]


def start_tau(tau0, nbin):
    """The fit's starting tau [rot]: tau0, or 1 / nbin where it is 0."""
    return tau0 if tau0 > 0.0 else 1.0 / nbin


def oracle_channel(data, model, nu, sigma, P, phi0, tau0, log10_tau):
    """The oracle's fit of one channel from (phi0, tau0 [rot, linear])."""
    nbin = len(data)
    t = start_tau(float(tau0), nbin)
    init = [float(phi0), 0.0, 0.0, np.log10(t) if log10_tau else t, 0.0]
    r = O.fit_portrait_full(data[None], model[None], init, P, np.array([nu]), [nu] * 3, [nu] * 3,
                            None if sigma is None else np.array([sigma]), FLAGS,
                            log10_tau=log10_tau)
    return dict(phi=r.phi, phi_err=r.phi_err, tau=r.tau, tau_err=r.tau_err, scale=r.scales[0],
                scale_err=r.scale_errs[0], snr=r.snr, red_chi2=r.red_chi2,
                cov=np.asarray(r.covariance_matrix), return_code=r.return_code,
                nfeval=r.nfeval)


def xcorr_phase(data, model, tau, nbin):
    """A starting phase for the oracle: the bin-resolution peak of the
    cross-correlation with the template scattered at tau."""
    B = O.scattering_portrait_FT(np.array([tau]), nbin)[0]
    X = np.fft.rfft(data) * np.conj(np.fft.rfft(model) * B)
    X[0] = 0.0
    ph = float(np.argmax(np.fft.irfft(X, nbin))) / nbin
    return (ph + 0.5) % 1.0 - 0.5
