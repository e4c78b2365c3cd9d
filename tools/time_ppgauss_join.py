"""Time a joint Gaussian-component fit of two receivers' portraits.

Two bands of 64 channels x 2048 bins (700-900 and 1100-1900 MHz) are
synthesised from three known components plus seeded noise, the second band
rotated by a phase and a DM offset.  Timed are

  joint    Engine.gauss_fit_join of the 128 x 2048 portrait with the flags
           DataPortrait sets (phase 0 fixed, every DM and the second phase
           free);
  nojoin   Engine.gauss_fit of the same 128 x 2048 portrait synthesised
           without the offsets (same noise), the cost without the feature;
  cpu_ref  scipy.optimize.leastsq with forward differences on the host
           residual of the joint problem, on one core: what the reference
           runs (--ref).

The device time is Engine.kernel_time("gauss") under Engine.set_timing (HIP
events around every launch of the fit); the wall time is the whole call
with its copies.  Each device fit runs --reps times after a warm-up call.

    python tools/time_ppgauss_join.py [--ref] [--reps 5] [--out times.json]
"""
import argparse
import importlib.util
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def yardstick():
    spec = importlib.util.spec_from_file_location(
        "make_golden_ppgauss_join",
        os.path.join(ROOT, "tests", "golden", "make_golden_ppgauss_join.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def components(ngauss, seed):
    rng = np.random.default_rng(seed)
    p = [0.01, 0.0]
    for loc in np.linspace(0.25, 0.75, ngauss):
        p += [loc, rng.uniform(-0.01, 0.01), rng.uniform(0.015, 0.04), rng.uniform(-0.5, 0.5),
              rng.uniform(0.3, 1.0), rng.uniform(-2.0, 0.0)]
    return np.array(p)


def timed(eng, reps, call):
    """(device ms, launches, wall s) per repeat, after one warm-up call."""
    call()
    recs = []
    for _ in range(reps):
        eng.set_timing(True)
        eng._chk(eng.lib.ppf_reset_kernel_times(eng.ctx))
        t0 = time.perf_counter()
        out = call()
        info = out["info"].cpu().numpy()  # ends in a device synchronise
        wall = time.perf_counter() - t0
        ms, launches = eng.kernel_time("gauss")
        eng.set_timing(False)
        recs.append((ms, int(launches), wall))
    return out, info, recs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", action="store_true", help="also time the CPU reference run")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from pulseportraiture_amd import pplib
    from pulseportraiture_amd.engine import get_engine
    YJ = yardstick()
    eng = get_engine(0)
    nchan, nbin, ngauss, P, nu_ref = 64, 2048, 3, 0.005, 1500.0
    freqs = np.concatenate([np.linspace(700.0, 900.0, nchan), np.linspace(1100.0, 1900.0, nchan)])
    groups = [np.arange(nchan), np.arange(nchan, 2 * nchan)]
    comps = components(ngauss, 1)
    p_join = np.concatenate([comps, [0.0, 0.0, 0.37, 3.0], [-4.0]])
    p_zero = np.concatenate([comps, [0.0, 0.0, 0.0, 0.0], [-4.0]])
    data, errs = YJ.synth("000", p_join, freqs, nbin, nu_ref, groups, P, 0.02, 10)
    data0, errs0 = YJ.synth("000", p_zero, freqs, nbin, nu_ref, groups, P, 0.02, 10)
    rng = np.random.default_rng(2)
    init = p_join.copy()
    init[:len(comps)] *= 1.0 + 0.01 * rng.uniform(-1, 1, len(comps))
    init[-5:-1] = [0.0, 0.0, 0.3702, 2.99]
    flags = np.ones(len(init), dtype=int)
    flags[[1, len(comps), -1]] = 0  # tau, the first phase, alpha
    join_of = YJ.join_of(groups, 2 * nchan)
    dm_coef = pplib.join_dm_coef(P, freqs, nu_ref)
    keep = np.r_[0:len(comps), len(init) - 1]
    results = []

    out, info, recs = timed(eng, args.reps, lambda: eng.gauss_fit_join(
        data, freqs, errs, init, flags, "000", nu_ref, join_of, dm_coef, 2))
    results.append(dict(
        what="joint", shape="2 x 64x2048_3", nfree=int(info[0, 3]), nfev=int(info[0, 1]),
        status=int(info[0, 0]), red_chi2=float(out["chi2"].cpu().numpy()[0] / info[0, 2]),
        join_params=[float(v) for v in out["params"].cpu().numpy()[0, -5:-1]],
        device_ms=[r[0] for r in recs], launches=recs[0][1], wall_s=[r[2] for r in recs]))
    print(json.dumps(results[-1]))

    out, info, recs = timed(eng, args.reps, lambda: eng.gauss_fit(
        data0, freqs, errs0, init[keep], flags[keep], "000", nu_ref))
    results.append(dict(
        what="nojoin", shape="128x2048_3", nfree=int(info[0, 3]), nfev=int(info[0, 1]),
        status=int(info[0, 0]), red_chi2=float(out["chi2"].cpu().numpy()[0] / info[0, 2]),
        device_ms=[r[0] for r in recs], launches=recs[0][1], wall_s=[r[2] for r in recs]))
    print(json.dumps(results[-1]))

    if args.ref:
        pr = YJ.Problem("000", data, errs, freqs, nu_ref, init, flags, groups, P)
        t0 = time.perf_counter()
        ref = pr.solve(False)
        results.append(dict(what="cpu_ref", shape="2 x 64x2048_3",
                            cpu_ref_s=time.perf_counter() - t0, nfev=int(ref["nfev"]),
                            ier=int(ref["ier"]), red_chi2=ref["chi2"] / ref["dof"],
                            join_params=[float(v) for v in ref["p"][-5:-1]]))
        print(json.dumps(results[-1]))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
