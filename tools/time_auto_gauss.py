"""Time the automatic Gaussian-component search on the device and its numpy +
scipy restatement on one core.

A three-component profile of nbin 2048 plus seeded noise is searched by
pplib.auto_gaussian_profiles, alone and as 64 such profiles (different noise)
in one call.  The device times are Engine.kernel_time("gbank") (the filter
bank) and Engine.kernel_time("gauss") (the Levenberg-Marquardt refits) under
Engine.set_timing (HIP events around every launch); the wall time is the
whole call.  --ref also runs tests/auto_gauss_reference.py's auto() on the
first profile with its bank in the correlation form (bank_fft): the only
yardstick, as the reference's step is a person at a plot.

    python tools/time_auto_gauss.py [--ref] [--out profiles/auto_gauss_times.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NBIN, SIGMA = 2048, 0.01
P_TRUE = [0.02, 0.0, 0.2, 0.03, 1.0, 0.5, 0.06, 0.5, 0.8, 0.015, 0.7]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", action="store_true", help="also time the CPU restatement")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from pulseportraiture_amd import pplib
    from pulseportraiture_amd.engine import get_engine
    eng = get_engine(0)
    clean = pplib.gen_gaussian_profile(P_TRUE, NBIN)
    profs = [clean + SIGMA * np.random.default_rng(100 + i).standard_normal(NBIN)
             for i in range(64)]
    results = []
    for nprof in (1, 64):
        for rep in range(2):  # the first pass allocates the workspace
            eng.set_timing(True)
            eng._chk(eng.lib.ppf_reset_kernel_times(eng.ctx))
            t0 = time.perf_counter()
            found = pplib.auto_gaussian_profiles(profs[:nprof], [SIGMA] * nprof)
            wall = time.perf_counter() - t0
            bank_ms, bank_n = eng.kernel_time("gbank")
            fit_ms, fit_n = eng.kernel_time("gauss")
            eng.set_timing(False)
        rec = dict(nbin=NBIN, nprof=nprof, ngauss=[int(f.ngauss) for f in found],
                   stages=[len(f.history) for f in found],
                   nfev=[int(f.lm_results.nfev) for f in found],
                   red_chi2=[float(f.chi2 / f.dof) for f in found],
                   bank_device_ms=bank_ms, bank_calls=int(bank_n), fit_device_ms=fit_ms,
                   fit_launch_groups=int(fit_n), wall_s=wall)
        print(json.dumps(rec))
        results.append(rec)
    if args.ref:
        from tests import auto_gauss_reference as R
        R.auto(profs[0][::8], SIGMA, bank=R.bank_fft)  # imports outside the clock
        t0 = time.perf_counter()
        a = R.auto(profs[0], SIGMA, bank=R.bank_fft)
        rec = dict(nbin=NBIN, nprof=1, cpu_restatement_s=time.perf_counter() - t0,
                   ngauss=int(a["ngauss"]), stages=len(a["history"]),
                   red_chi2=a["chi2"] / a["dof"])
        print(json.dumps(rec))
        results.append(rec)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
