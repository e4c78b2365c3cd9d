#!/usr/bin/env python3
"""The reference's wideband fit at profile lengths that are no power of two
(generic_nbin.npz).

TEST INFRASTRUCTURE ONLY -- run in the build container, never on the GPU box
and never by the product.  The reference is loaded through the shim of
make_golden.py, as in make_golden_nb_scat_odd.py; only numbers are written.

Every other wideband fixture is at nbin 2048 or another power of two.  Here
two cases, nbin 1000 and 1536 (both even, so the reference's irfft without a
length is harmless), each 2 subints x 8 channels of synth.make_workload, are
fitted for phi and DM with get_TOAs' per-subint flow and the reference's own
functions (pptoas.py:383-488): get_noise per channel, guess_fit_freq with
SNRs 1, the phase guess (pptoas.py:420-456), then
pptoaslib.fit_portrait_full (trust-ncg, fit_flags [1, 1, 0, 0, 0], option 0).

generic_nbin.npz, per case c0 / c1: data [2, 8, nbin], model [8, nbin], freqs
[8], P, errs [2, 8], init [2, 5], nu_fit [2], and the reference's phi,
phi_err, DM, DM_err, nu_DM, red_chi2, snr, return_code, nfeval [2].

Before it writes, the script checks that the oracle (oracle/ppfit_oracle.py)
lies within half of each bar of tests/test_row_fft_cpu.py and
tests/test_gpu_row_fft.py against the reference -- 0.5e-3 sigma on phi and DM,
0.5e-4 relative on their errors, 0.5e-6 on red_chi2, the same return code --
so no subint needs an "alternative end point"; if one does not, change that
case's SEED.

Usage:  python tests/golden/make_golden_generic_nbin.py
"""
import contextlib
import io
import os
import shutil
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import make_golden as MG  # noqa: E402
from oracle import ppfit_oracle as O  # noqa: E402
from pulseportraiture_amd import synth  # noqa: E402

NSUB, NCHAN, FLAGS = 2, 8, [1, 1, 0, 0, 0]
CASES = [(1000, 771000), (1536, 771536)]  # (nbin, SEED)
REF = ["phi", "phi_err", "DM", "DM_err", "nu_DM", "red_chi2", "snr", "return_code", "nfeval"]


def gen(pplib, pptoaslib):
    out = {}
    for ic, (nbin, seed) in enumerate(CASES):
        w = synth.make_workload(NSUB, NCHAN, nbin, seed=seed)
        data = synth.workload_data_host(w)
        rows = {k: [] for k in REF}
        errs_all, inits, nu_fits = [], [], []
        for i in range(NSUB):
            port = data[i]
            errs = np.asarray(pplib.get_noise(port, chans=True))
            nu_fit = float(pplib.guess_fit_freq(w.freqs, np.ones(NCHAN)))
            nu_mean = w.freqs.mean()
            rot = pplib.rotate_data(port, 0.0, w.DM0, w.P, w.freqs, nu_mean)
            prof = np.average(rot, axis=0, weights=np.ones(NCHAN))
            phi_g = pplib.fit_phase_shift(prof, w.model.mean(axis=0), Ns=100).phase
            phi_g = float(pplib.phase_transform(phi_g, w.DM0, nu_mean, nu_fit, w.P, mod=True))
            init = [phi_g, w.DM0, 0.0, 0.0, 0.0]
            with contextlib.redirect_stdout(io.StringIO()):
                r = pptoaslib.fit_portrait_full(port, w.model, list(init), w.P, w.freqs,
                                                [nu_fit] * 3, [None] * 3, errs, list(FLAGS),
                                                None, False, option=0, sub_id=None,
                                                method="trust-ncg", is_toa=True, quiet=True)
            ref = dict(phi=r.phi, phi_err=r.phi_err, DM=r.DM, DM_err=r.DM_err, nu_DM=r.nu_DM,
                       red_chi2=r.red_chi2, snr=r.snr, return_code=r.return_code,
                       nfeval=r.nfeval)
            for k in REF:
                rows[k].append(float(ref[k]))
            errs_all.append(errs)
            inits.append(init)
            nu_fits.append(nu_fit)
            o = O.fit_portrait_full(port, w.model, list(init), w.P, w.freqs, [nu_fit] * 3,
                                    [None] * 3, errs, list(FLAGS), log10_tau=False,
                                    method="trust-ncg")
            sig = max(abs(o.phi - r.phi) / r.phi_err, abs(o.DM - r.DM) / r.DM_err)
            rel = max(abs(o.phi_err / r.phi_err - 1.0), abs(o.DM_err / r.DM_err - 1.0))
            chi = abs(o.red_chi2 / r.red_chi2 - 1.0)
            print("  nbin %d subint %d: oracle - reference %.3g sigma, errors %.3g, red_chi2 "
                  "%.3g relative, rc %d / %d, snr %.1f" % (nbin, i, sig, rel, chi, o.return_code,
                                                           r.return_code, r.snr))
            assert sig <= 0.5e-3 and rel <= 0.5e-4 and chi <= 0.5e-6 and \
                o.return_code == r.return_code, "nbin %d subint %d: change SEED %d" % (nbin, i, seed)
        key = "c%d_" % ic
        out[key + "nbin"] = np.array(nbin)
        out[key + "seed"] = np.array(seed)
        out[key + "data"] = data
        out[key + "model"] = w.model
        out[key + "freqs"] = w.freqs
        out[key + "P"] = np.array(w.P)
        out[key + "errs"] = np.array(errs_all)
        out[key + "init"] = np.array(inits)
        out[key + "nu_fit"] = np.array(nu_fits)
        for k in REF:
            out[key + k] = np.array(rows[k])
    return out


def main():
    tmp, pplib, pptoaslib, _, _ = MG.load_reference()
    try:
        out = gen(pplib, pptoaslib)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    MG.save("generic_nbin.npz", **out)
    assert os.path.getsize(os.path.join(HERE, "generic_nbin.npz")) < 600 * 1024


if __name__ == "__main__":
    main()
