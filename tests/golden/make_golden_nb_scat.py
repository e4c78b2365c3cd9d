#!/usr/bin/env python3
"""Golden fixture for get_narrowband_TOAs(fit_scat=True): a phase and a
scattering time per channel.

TEST INFRASTRUCTURE ONLY -- run in the build container, never on the GPU box
and never by the product.  The reference is loaded through the shim of
make_golden.py, as in make_golden_r2.py; only numbers are written.

The reference's narrowband driver leaves its per-channel scattering fit
commented out (pptoas.py:752-753, 982-988), so the fixture runs what that
call stands for: pptoaslib.fit_portrait_full on each channel as a one-channel
portrait with fit_flags [1, 0, 0, 1, 0] and nu_fits = nu_outs = the channel's
frequency, method trust-ncg.

nb_scat.npz, per case c<i>_ (channels along the first axis):
  data, model      the channel rows and the unscattered template rows
  freqs, errs      channel frequency [MHz], noise sigma (pplib.get_noise)
  tau0             the starting tau [rot] at the channel's frequency, linear
                   (0: the fit starts at 1 / nbin)
  phi0             the reference's starting phase
  phi, phi_err, tau, tau_err, scale, scale_err, snr, red_chi2, cov [2, 2],
  return_code, nfeval     the reference's results (tau: the fitted parameter)
  nbin, tau_inj, log10    the case
and P, ncase.

Usage:  python tests/golden/make_golden_nb_scat.py
"""
import os
import shutil
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import make_golden as MG  # noqa: E402
from make_golden_r2 import quiet_call  # noqa: E402

P0 = MG.P0

CASES = [
    # (nchan, nbin, tau injected at 1500 MHz [rot], log10_tau, noise sigma)
    (16, 64, 2e-2, True, 0.04),
    (16, 256, 4e-3, True, 0.08),
    (16, 256, 4e-3, False, 0.08),
    (16, 512, 1e-2, True, 0.08),
    (8, 2048, 2e-3, True, 0.15),
    (16, 100, 1e-2, True, 0.018),
    (8, 256, 0.0, True, 0.04),
]
ALPHA = -4.0
BW = 200.0
MIN_SNR = 15.0


def start_phase(pplib, prof, tmpl, tau, nbin):
    """The bin-resolution peak of the cross-correlation between the profile
    and the template scattered at tau, as a phase in [-0.5, 0.5)."""
    B = pplib.scattering_portrait_FT(np.array([tau]), nbin)[0]
    X = np.fft.rfft(prof) * np.conj(np.fft.rfft(tmpl) * B)
    X[0] = 0.0
    cc = np.fft.irfft(X, nbin)
    ph = float(np.argmax(cc)) / nbin  # cc[j] = sum_k Re(X_k e^{2 pi i k j / nbin})
    return (ph + 0.5) % 1.0 - 0.5


def make_portrait(ref, rng, nchan, nbin, phi, dDM, noise, tau):
    """make_golden.make_portrait over BW MHz around 1500 MHz, so that tau
    (alpha = -4) stays measurable in every channel."""
    pplib, pptoaslib = ref
    freqs = MG.channel_freqs(nchan, 1500.0, BW)
    _, _, model = pplib.read_model(MG.GMODEL, pplib.get_bin_centers(nbin), freqs, P0, quiet=True)
    m = model
    if tau:
        taus = pplib.scattering_times(tau, ALPHA, freqs, 1500.0)
        m = np.fft.irfft(pplib.scattering_portrait_FT(taus, nbin) * np.fft.rfft(m, axis=-1),
                         axis=-1)
    data = pptoaslib.rotate_portrait_full(m, -phi, -(MG.DM0 + dDM), 0.0, freqs, 1500.0, np.inf,
                                          P0)
    return freqs, model, data + rng.normal(0.0, noise, data.shape)


def gen(pplib, pptoaslib):
    rng = np.random.default_rng(97531)
    out, low = {}, []
    for ic, (nchan, nbin, tau, log10_tau, noise) in enumerate(CASES):
        phi = rng.uniform(-0.1, 0.1)
        dDM = rng.normal(3e-4, 2e-4)
        freqs, model, data = make_portrait((pplib, pptoaslib), rng, nchan, nbin, phi, dDM,
                                           noise, tau)
        errs = pplib.get_noise(data, chans=True)
        # a start 30 % off the injected value, scaled to each channel
        tau0 = 0.7 * tau * (freqs / 1500.0) ** ALPHA
        rows = {k: [] for k in ["phi0", "phi", "phi_err", "tau", "tau_err", "scale", "scale_err",
                                "snr", "red_chi2", "cov", "return_code", "nfeval"]}
        for n in range(nchan):
            t_lin = tau0[n] if tau0[n] else 1.0 / nbin
            phi0 = start_phase(pplib, data[n], model[n], t_lin, nbin)
            init = [phi0, 0.0, 0.0, np.log10(t_lin) if log10_tau else t_lin, 0.0]
            nu = freqs[n]
            r = quiet_call(pptoaslib.fit_portrait_full, data[n:n + 1], model[n:n + 1], init, P0,
                           freqs[n:n + 1], [nu, nu, nu], [nu, nu, nu], errs[n:n + 1],
                           [1, 0, 0, 1, 0], None, log10_tau, option=0, method="trust-ncg")
            cov = np.asarray(r.covariance_matrix, dtype=float)
            assert cov.shape == (2, 2), cov.shape
            rows["phi0"].append(phi0)
            rows["phi"].append(float(r.phi))
            rows["phi_err"].append(float(r.phi_err))
            rows["tau"].append(float(r.tau))
            rows["tau_err"].append(float(r.tau_err))
            rows["scale"].append(float(r.scales[0]))
            rows["scale_err"].append(float(r.scale_errs[0]))
            rows["snr"].append(float(r.snr))
            rows["red_chi2"].append(float(r.red_chi2))
            rows["cov"].append(cov)
            rows["return_code"].append(int(r.return_code))
            rows["nfeval"].append(int(r.nfeval))
        key = "c%d_" % ic
        out[key + "data"] = data
        out[key + "model"] = model
        out[key + "freqs"] = freqs
        out[key + "errs"] = errs
        out[key + "tau0"] = tau0
        out[key + "nbin"] = np.array(nbin)
        out[key + "tau_inj"] = np.array(tau)
        out[key + "log10"] = np.array(log10_tau)
        for k, v in rows.items():
            out[key + k] = np.array(v)
        snr = np.array(rows["snr"])
        print("case %d nbin %d tau %g log10 %d: snr %.1f..%.1f rc %s nfev %d..%d" % (
            ic, nbin, tau, log10_tau, snr.min(), snr.max(), sorted(set(rows["return_code"])),
            min(rows["nfeval"]), max(rows["nfeval"])))
        low.append(snr.min())
    assert min(low) >= MIN_SNR, "S/N below %g: %s" % (MIN_SNR, low)
    out["ncase"] = np.array(len(CASES))
    out["P"] = np.array(P0)
    MG.save("nb_scat.npz", **out)


def main():
    np.seterr(all="ignore")
    tmp, pplib, pptoaslib, _, _ = MG.load_reference()
    try:
        gen(pplib, pptoaslib)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
