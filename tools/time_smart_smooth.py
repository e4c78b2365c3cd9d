"""Time smart_smooth (wavelet smoothing, ppfit_swt.hip) on the device.

Three workloads, nbin 2048:
  - one model: the ten leading eigenvectors and the mean profile of a 64-channel
    portrait (what make_spline_model(smooth="swt") smooths), 11 rows;
  - 16 such models' rows in one call (make_spline_models), 176 rows;
  - DataPortrait.smooth_portrait(smart=True) of a 512-channel portrait (8
    levels; the portrait and its unzapped channels, 2 x 512 rows).
It also records which eigenvectors of a 64 x 1024 portrait make_spline_model
takes as significant with smooth=False and with smooth="swt".
The device time is Engine.kernel_time("swt") under Engine.set_timing (HIP
events around every launch), the wall time is the whole call.  --ref also
times the numpy restatement of the same search (tests/swt_reference.py, one
core) on the first workload.  That restatement is plain numpy; PyWavelets' C
code, which the reference uses, would be faster and is not what is timed.

    python tools/time_smart_smooth.py [--ref] [--out profiles/smart_smooth_times.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NBIN = 2048


def portrait(nchan, seed, sigma=0.02, nbin=NBIN):
    rng = np.random.default_rng(seed)
    t = np.arange(nbin) / nbin
    freqs = np.linspace(1100.0, 1900.0, nchan)
    x = (freqs - 1500.0) / 400.0
    s1 = np.exp(-0.5 * ((t - 0.3) / 0.04) ** 2)
    s2 = np.exp(-0.5 * ((t - 0.45) / 0.02) ** 2)
    port = (np.outer(1.0 + 0.5 * x, s1) + np.outer(0.4 + 0.3 * x ** 2 - 0.2 * x, s2)
            + sigma * rng.standard_normal((nchan, nbin)))
    return freqs, port, sigma


def archive(nchan, seed, name, nbin=NBIN):
    from pulseportraiture_amd.mjd import MJD
    freqs, port, sigma = portrait(nchan, seed, nbin=nbin)
    snrs = np.sqrt((port ** 2).sum(axis=1)) / sigma
    return dict(subints=port[None, None], freqs=freqs[None], weights=np.ones((1, nchan)),
                SNRs=snrs[None, None], noise_stds=np.full((1, 1, nchan), sigma), Ps=[0.003],
                epochs=[MJD(57300.0)], bw=800.0, source="J0000+0000", filename=name)


def model_rows(eng, nmodel):
    """The rows make_spline_models smooths for nmodel 64-channel portraits."""
    ports = np.stack([portrait(64, 20 + i)[1] for i in range(nmodel)])
    w = np.sqrt((ports ** 2).sum(axis=2))
    mean, _, eigvec, _ = eng.pca_portraits(ports, w / w.sum(axis=1, keepdims=True), 10)
    return np.concatenate([eigvec.cpu().numpy().reshape(-1, NBIN), mean.cpu().numpy()])


def timed(eng, call):
    for rep in range(2):  # the first pass allocates the workspace
        eng.set_timing(True)
        eng._chk(eng.lib.ppf_reset_kernel_times(eng.ctx))
        t0 = time.perf_counter()
        out = call()
        wall = time.perf_counter() - t0
        ms, launches = eng.kernel_time("swt")
        eng.set_timing(False)
    return out, dict(device_ms=ms, launches=int(launches), wall_s=wall)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", action="store_true", help="also time the numpy restatement")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from pulseportraiture_amd import pplib, ppspline
    from pulseportraiture_amd.engine import get_engine
    eng = get_engine(0)
    results = []
    first = None
    for label, nmodel in (("1 model: 11 x 2048", 1), ("16 models: 176 x 2048", 16)):
        rows = model_rows(eng, nmodel)
        res, rec = timed(eng, lambda: pplib.smart_smooth(rows, full=True))
        rec = dict(workload=label, nrow=len(rows), nbin=NBIN, levels=11,
                   nlevel=[int(v) for v in res["nlevel"]][:11],
                   zeroed=[int(v) for v in res["zeroed"]][:11], **rec)
        print(json.dumps(rec))
        results.append(rec)
        if first is None:
            first = rows
    arch = archive(512, 5, "smooth_portrait.fits")

    dps = iter([ppspline.DataPortrait(arch, quiet=True) for rep in range(2)])
    _, rec = timed(eng, lambda: next(dps).smooth_portrait(smart=True))
    rec = dict(workload="smooth_portrait(smart=True): 2 x 512 x 2048", nrow=1024, nbin=NBIN,
               levels=8, **rec)
    print(json.dumps(rec))
    results.append(rec)
    # which eigenvectors of a 64 x 1024 portrait pass the S/N test either way
    ieig = {}
    for smooth in (False, "swt"):
        dp = ppspline.DataPortrait(archive(64, 7, "select.fits", nbin=1024), quiet=True)
        dp.make_spline_model(smooth=smooth, quiet=True)
        ieig[smooth] = [int(i) for i in dp.ieig]
    rec = dict(workload="make_spline_model 64 x 1024", ieig_unsmoothed=ieig[False],
               ieig_swt=ieig["swt"])
    print(json.dumps(rec))
    results.append(rec)
    if args.ref:
        from tests import swt_reference as R
        t0 = time.perf_counter()
        for row in first:
            R.smart_smooth(row)
        rec = dict(workload="1 model: 11 x 2048",
                   numpy_restatement_one_core_s=time.perf_counter() - t0)
        print(json.dumps(rec))
        results.append(rec)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
