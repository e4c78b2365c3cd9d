#!/usr/bin/env python3
"""Generate the noise-fit fixtures from the reference PulsePortraiture source.

TEST INFRASTRUCTURE ONLY, run in the build container like make_golden.py,
whose shim (load_reference) it reuses.  The reference's get_noise_fit,
find_kc, find_kc_function, get_noise_PS and get_SNR run on seeded rows: a
Gaussian pulse (FWHM 0.002 / 0.02 / 0.2 in phase, peak S/N 0 / 1 / 30 / 1000)
in unit white noise at nbin 16, 64, 250, 256 and 2048, an all-zero row, a
spectrum whose DC power is exactly zero, a two-row portrait (chans=False),
half_tri and weighted searches.

For every row the best objective per decay rate `a` is recorded (the
reference's find_kc_function on scipy brute's own grid), with the relative gap
between the two smallest of those twenty minima: a row is `separated` -- its
kc safe from rounding -- if the gap exceeds 1e-9 or the minima tie exactly on
the b = 0 plane.  Tests compare kc on separated rows only; fewer than 90 % of
them separated fails this script, so the filter cannot hide a failure.

Only numbers are written: tests/golden/noise_fit.npz.

Usage:  python tests/golden/make_golden_noise_fit.py
"""
import os
import shutil
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import make_golden  # noqa: E402

NBINS = (16, 64, 250, 256, 2048)
WIDTHS = (0.002, 0.02, 0.2)
SNRS = (0.0, 1.0, 30.0, 1000.0)
NS = 20
GAP = 1e-9


def make_row(nbin, width, snr, seed):
    rng = np.random.default_rng(seed)
    ph = (np.arange(nbin) + 0.5) / nbin
    sig = width / (2.0 * np.sqrt(2.0 * np.log(2.0)))
    return snr * np.exp(-0.5 * ((ph - 0.5) / sig) ** 2) + rng.standard_normal(nbin)


def power_spectrum(row):
    X = np.fft.rfft(row)
    return np.real(X * np.conj(X)) / len(row)


def per_a_minima(pplib, pows, errs=1.0, fn="exp_dc"):
    """The best find_kc_function value per a on brute's grid, and the flat
    index of the overall winner."""
    d = np.log10(pows)
    n = len(d)
    lo, hi = (1.0 / n, 1.0) if fn == "exp_dc" else (1, n)
    grid = np.mgrid[slice(lo, hi, complex(NS)), slice(0, d.max() - d.min(), complex(NS)),
                    slice(d.min(), d.max(), complex(NS))]
    S = np.empty((NS, NS, NS))
    for ia in range(NS):
        for ib in range(NS):
            for ic in range(NS):
                S[ia, ib, ic] = pplib.find_kc_function(grid[:, ia, ib, ic], d, errs, fn)
    return S.reshape(NS, -1).min(axis=1), int(np.argmin(S))


def gap_of(per_a):
    s = np.sort(per_a)
    return (s[1] - s[0]) / abs(s[1]) if np.isfinite(s[:2]).all() and s[1] != 0 else np.nan


def main():
    tmp, pplib, _, _, _ = make_golden.load_reference()
    np.seterr(all="ignore")
    out = {}
    # --- seeded rows, one array per nbin ---------------------------------
    nsep = ntot = 0
    for nbin in NBINS:
        rows, meta, kcs, noises, per_as, idxs, seps = [], [], [], [], [], [], []
        for iw, width in enumerate(WIDTHS):
            for isn, snr in enumerate(SNRS):
                row = make_row(nbin, width, snr, 1000 * nbin + 10 * iw + isn)
                pows = power_spectrum(row)
                kc = int(pplib.find_kc(pows))
                per_a, idx = per_a_minima(pplib, pows)
                s = np.sort(per_a)
                sep = bool(gap_of(per_a) > GAP or (s[0] == s[1] and (idx // NS) % NS == 0))
                rows.append(row)
                meta.append([width, snr])
                kcs.append(kc)
                noises.append(float(pplib.get_noise_fit(row)))
                per_as.append(per_a)
                idxs.append(idx)
                seps.append(sep)
                nsep += sep
                ntot += 1
        k = "_%d" % nbin
        out["rows" + k] = np.array(rows)
        out["meta" + k] = np.array(meta)
        out["kc" + k] = np.array(kcs, dtype=np.int64)
        out["noise" + k] = np.array(noises)
        out["per_a" + k] = np.array(per_as)
        out["idx" + k] = np.array(idxs, dtype=np.int64)
        out["gap" + k] = np.array([gap_of(p) for p in per_as])
        out["separated" + k] = np.array(seps)
        out["noise_chans" + k] = pplib.get_noise_fit(np.array(rows), chans=True)
        out["noise_fact2" + k] = pplib.get_noise_fit(np.array(rows), fact=2.0, chans=True)
        out["ps2" + k] = pplib.get_noise_PS(np.array(rows), frac=2, chans=True)
        out["ps8" + k] = pplib.get_noise_PS(np.array(rows), frac=8, chans=True)
        print("nbin", nbin, "kc", kcs, "separated", int(np.sum(seps)), "of", len(seps))
    print("separated: %d of %d rows" % (nsep, ntot))
    assert nsep >= 0.9 * ntot, "fewer than 90 % of the rows are separated"
    out["nbins"] = np.array(NBINS)
    # --- zero-power rows ------------------------------------------------------
    zero = np.zeros(64)
    out["zero_row"] = zero
    out["zero_noise"] = np.array(float(pplib.get_noise_fit(zero)))
    out["zero_kc"] = np.array(int(pplib.find_kc(power_spectrum(zero))))
    zdc = power_spectrum(make_row(256, 0.02, 30.0, 77))
    zdc[0] = 0.0
    out["zero_dc_pows"] = zdc
    out["zero_dc_kc"] = np.array(int(pplib.find_kc(zdc)))
    # --- a portrait, chans=False (the ravelled rows are one profile) ----------
    port = np.array([make_row(128, 0.02, 30.0, 78), make_row(128, 0.02, 10.0, 79)])
    out["port"] = port
    out["port_noise_fit"] = np.array(float(pplib.get_noise_fit(port)))
    out["port_noise_fit_chans"] = pplib.get_noise_fit(port, chans=True)
    out["port_noise_ps2"] = np.array(float(pplib.get_noise_PS(port, frac=2)))
    out["port_noise_ps8"] = np.array(float(pplib.get_noise_PS(port, frac=8)))
    # --- half_tri and weighted searches ---------------------------------------
    spectra = [power_spectrum(make_row(nbin, w, s, 500 + i))
               for i, (nbin, w, s) in enumerate([(64, 0.2, 30.0), (250, 0.02, 1000.0),
                                                 (256, 0.02, 30.0), (256, 0.002, 1000.0)])]
    for i, p in enumerate(spectra):
        out["ht_pows_%d" % i] = p
        out["ht_kc_%d" % i] = np.array(int(pplib.find_kc(p, fn="half_tri")))
        per_a, idx = per_a_minima(pplib, p, fn="half_tri")
        out["ht_per_a_%d" % i], out["ht_idx_%d" % i] = per_a, np.array(idx)
        errs = 0.5 + np.random.default_rng(600 + i).uniform(0.0, 1.0, len(p))
        out["w_errs_%d" % i] = errs
        out["w_kc_%d" % i] = np.array(int(pplib.find_kc(p, errs=errs)))
        per_a, idx = per_a_minima(pplib, p, errs=errs)
        out["w_per_a_%d" % i], out["w_idx_%d" % i] = per_a, np.array(idx)
        out["w_ht_kc_%d" % i] = np.array(int(pplib.find_kc(p, errs=errs, fn="half_tri")))
        per_a, idx = per_a_minima(pplib, p, errs=errs, fn="half_tri")
        out["w_ht_per_a_%d" % i], out["w_ht_idx_%d" % i] = per_a, np.array(idx)
    out["n_spectra"] = np.array(len(spectra))
    # --- get_SNR (default noise method) on six baseline-free profiles ----------
    profs = [make_row(nbin, w, s, 700 + i)
             for i, (nbin, w, s) in enumerate([(64, 0.2, 30.0), (250, 0.02, 30.0),
                                               (256, 0.02, 1000.0), (256, 0.2, 1.0),
                                               (2048, 0.02, 30.0), (2048, 0.002, 1000.0)])]
    for i, p in enumerate(profs):
        out["snr_prof_%d" % i] = p
        out["snr_%d" % i] = np.array(float(pplib.get_SNR(p)))
        out["snr_fudge1_%d" % i] = np.array(float(pplib.get_SNR(p, fudge=1.0)))
    out["n_snr"] = np.array(len(profs))
    make_golden.save("noise_fit.npz", **out)
    assert os.path.getsize(os.path.join(HERE, "noise_fit.npz")) < (1 << 20)
    shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
