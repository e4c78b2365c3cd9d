#!/usr/bin/env python3
"""Golden fixture for the narrowband phase + tau fit at odd profile lengths.

TEST INFRASTRUCTURE ONLY -- run in the build container, never on the GPU box
and never by the product.  The reference is loaded through the shim of
make_golden.py, as in make_golden_nb_scat.py; only numbers are written.

An odd nbin has no Nyquist term, errs_FT = sigma sqrt(nbin / 2) with a
half-integer under the root and dof = nbin - 3 odd; nb_scat.npz holds no such
length.  The reference's own data builders call irfft without a length, which
returns nbin - 1 samples for an odd nbin, so the rows are built by
tests/test_gpu_nb_scat.gaussian_channel, which passes nbin to irfft: a
two-Gaussian template scattered by tau and rotated by -phi, plus white noise.
The only reference code called is pptoaslib.fit_portrait_full, exactly as
make_golden_nb_scat.py calls it (one-channel portrait, fit_flags
[1, 0, 0, 1, 0], nu_fits = nu_outs = the channel's frequency, trust-ncg), with
the noise level given.

nb_scat_odd.npz: the keys of nb_scat.npz (see make_golden_nb_scat.py); each
case holds four rows with their own seed and injected phase.

The rows are chosen so that the oracle (tests/nb_scat_cases.oracle_channel)
stays within half of each bar of tests/test_nb_scat_golden_cpu.py against the
reference; this script checks that before it writes and names the row that
does not.

Usage:  python tests/golden/make_golden_nb_scat_odd.py
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
from make_golden_nb_scat import start_phase  # noqa: E402
from make_golden_r2 import quiet_call  # noqa: E402

P0 = MG.P0
NU = 1400.0
SIGMA = 0.05
MIN_SNR = 15.0

CASES = [
    # (nbin, log10_tau, [(seed, injected phase) per row])
    (999, True, [(1999, 0.137), (2999, -0.31), (3999, 0.052), (4999, 0.44)]),
    (2049, False, [(12049, -0.137), (22049, 0.21), (32049, -0.46), (42049, 0.003)]),
]


def shape_of(nbin):
    """(width, tau) [rot] of the rows, as test_slot_and_length_seams."""
    width = max(0.004, 4.0 / nbin)
    return width, 0.75 * width


def gen(pplib, pptoaslib):
    from tests import nb_scat_cases as NB
    from tests.test_gpu_nb_scat import gaussian_channel
    out, low = {}, []
    for ic, (nbin, log10_tau, rows_in) in enumerate(CASES):
        width, tau = shape_of(nbin)
        built = [gaussian_channel(nbin, width, tau, phi, SIGMA, seed) for seed, phi in rows_in]
        model = np.stack([b[0] for b in built])
        data = np.concatenate([b[1] for b in built])
        nrow = len(rows_in)
        freqs = np.full(nrow, NU)
        errs = np.full(nrow, SIGMA)
        tau0 = np.full(nrow, 0.6 * tau)
        rows = {k: [] for k in ["phi0", "phi", "phi_err", "tau", "tau_err", "scale", "scale_err",
                                "snr", "red_chi2", "cov", "return_code", "nfeval"]}
        for n in range(nrow):
            phi0 = start_phase(pplib, data[n], model[n], tau0[n], nbin)
            init = [phi0, 0.0, 0.0, np.log10(tau0[n]) if log10_tau else tau0[n], 0.0]
            r = quiet_call(pptoaslib.fit_portrait_full, data[n:n + 1], model[n:n + 1], init, P0,
                           freqs[n:n + 1], [NU, NU, NU], [NU, NU, NU], errs[n:n + 1],
                           [1, 0, 0, 1, 0], None, log10_tau, option=0, method="trust-ncg")
            cov = np.asarray(r.covariance_matrix, dtype=float)
            assert cov.shape == (2, 2), cov.shape
            ref = dict(phi0=phi0, phi=float(r.phi), phi_err=float(r.phi_err), tau=float(r.tau),
                       tau_err=float(r.tau_err), scale=float(r.scales[0]),
                       scale_err=float(r.scale_errs[0]), snr=float(r.snr),
                       red_chi2=float(r.red_chi2), cov=cov, return_code=int(r.return_code),
                       nfeval=int(r.nfeval))
            for k, v in ref.items():
                rows[k].append(v)
            # the oracle against the reference: half of each bar of
            # tests/test_nb_scat_golden_cpu.py
            o = NB.oracle_channel(data[n], model[n], NU, SIGMA, P0, phi0, tau0[n], log10_tau)
            sig = max(abs(o["phi"] - ref["phi"]) / ref["phi_err"],
                      abs(o["tau"] - ref["tau"]) / ref["tau_err"])
            rel = max([abs(o[k] / ref[k] - 1.0) for k in ["phi_err", "tau_err", "scale",
                                                          "scale_err", "snr", "red_chi2"]]
                      + [np.abs(o["cov"] / cov - 1.0).max()])
            print("  nbin %d row %d (seed %d): oracle - reference %.3g sigma, %.3g relative, "
                  "rc %d / %d" % (nbin, n, rows_in[n][0], sig, rel, o["return_code"],
                                  ref["return_code"]))
            assert sig <= 0.5e-4 and rel <= 0.5e-6 and o["return_code"] == ref["return_code"], \
                "nbin %d row %d: change its seed" % (nbin, n)
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
    MG.save("nb_scat_odd.npz", **out)


def main():
    np.seterr(all="ignore")
    tmp, pplib, pptoaslib, _, _ = MG.load_reference()
    try:
        gen(pplib, pptoaslib)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
