"""Time ppgauss model fits on the device and the CPU yardstick's reference run.

For each shape a portrait is synthesised from known components plus seeded
noise and fitted by ppgauss.make_gaussian_model from a perturbed model file;
the device time is Engine.kernel_time("gauss") under Engine.set_timing (HIP
events around every launch of the fit), the wall time is the whole fit call.
--ref also runs scipy.optimize.leastsq with forward differences on the host
residual (what the reference does) for the first shape.

    python tools/time_ppgauss.py [--ref] [--out profiles/ppgauss_times.json]
"""
import argparse
import importlib.util
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def yardstick():
    spec = importlib.util.spec_from_file_location(
        "make_golden_ppgauss", os.path.join(ROOT, "tests", "golden", "make_golden_ppgauss.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def components(ngauss, seed):
    rng = np.random.default_rng(seed)
    p = [0.01, 0.0]
    for loc in np.linspace(0.25, 0.75, ngauss):
        p += [loc, rng.uniform(-0.01, 0.01), rng.uniform(0.015, 0.04), rng.uniform(-0.5, 0.5),
              rng.uniform(0.3, 1.0), rng.uniform(-2.0, 0.0)]
    return np.array(p + [-4.0])


def archive(Y, p, nchan, nbin, seed, name):
    from pulseportraiture_amd.mjd import MJD
    freqs, port, errs = Y.synth("000", p, nchan, nbin, 1500.0, 0.02, seed)
    return dict(subints=port[None, None], freqs=freqs[None], weights=np.ones((1, nchan)),
                SNRs=(port.max(axis=1) / errs)[None, None], noise_stds=errs[None, None],
                Ps=[0.003], epochs=[MJD(57300.0)], bw=800.0, nu0=1500.0, source="J0000+0000",
                filename=name), (freqs, port, errs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", action="store_true", help="also time the CPU reference run")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from pulseportraiture_amd import ppgauss, pplib
    from pulseportraiture_amd.engine import get_engine
    Y = yardstick()
    eng = get_engine(0)
    tmp = tempfile.mkdtemp()
    results = []
    for label, nchan, nbin, ngauss, nport in (("64x2048_3", 64, 2048, 3, 1),
                                              ("512x2048_10", 512, 2048, 10, 1),
                                              ("16 x 64x2048_3", 64, 2048, 3, 16)):
        p = components(ngauss, 1)
        init = p * (1.0 + 0.01 * np.random.default_rng(2).uniform(-1, 1, len(p)))
        start = os.path.join(tmp, "start_%d.gmodel" % ngauss)
        flags = np.ones(len(p) - 1, dtype=int)
        flags[1] = 0
        pplib.write_model(start, "start", "000", 1500.0, init[:-1], flags, -4.0, 0, quiet=True)
        made = [archive(Y, p, nchan, nbin, 10 + i, "t%d.fits" % i) for i in range(nport)]
        dps = [ppgauss.DataPortrait(a, quiet=True) for a, _ in made]
        for rep in range(2):  # the first pass allocates the workspace
            for dp in dps:
                dp.init_params = []
            eng.set_timing(True)
            eng._chk(eng.lib.ppf_reset_kernel_times(eng.ctx))
            t0 = time.perf_counter()
            ppgauss.make_gaussian_models(dps, modelfiles=[start] * nport, quiet=True)
            wall = time.perf_counter() - t0
            ms, launches = eng.kernel_time("gauss")
            eng.set_timing(False)
        rec = dict(shape=label, nchan=nchan, nbin=nbin, ngauss=ngauss, nport=nport,
                   nfree=int(np.sum(dps[0].fit_flags)),
                   nfev=[int(dp.fgp.lm_results.nfev) for dp in dps],
                   status=[int(dp.fgp.lm_results.status) for dp in dps],
                   red_chi2=[float(dp.chi2 / dp.dof) for dp in dps],
                   device_ms=ms, launches=int(launches), wall_s=wall,
                   fit_wall_s=float(sum(dp.total_time for dp in dps)))
        print(json.dumps(rec))
        results.append(rec)
        if args.ref and label == "64x2048_3":
            freqs, port, errs = made[0][1]
            pr = Y.Problem("000", port, errs, freqs, 1500.0, init, np.append(flags, 0))
            t0 = time.perf_counter()
            ref = pr.solve(False)
            rec = dict(shape=label, cpu_ref_s=time.perf_counter() - t0, nfev=int(ref["nfev"]),
                       ier=int(ref["ier"]), red_chi2=ref["chi2"] / ref["dof"])
            print(json.dumps(rec))
            results.append(rec)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
