"""Time get_noise_fit (ppf_noise_fit_rows, ppfit_noisefit.hip) on the device.

Workloads (a Gaussian pulse of FWHM 0.02, peak S/N 30, in unit white noise,
made on the device):
  - 64 x 2048 and 512 x 1024 rows in one call;
  - 640,000 x 2048 rows (a 10,000 x 64 archive) in chunks of 64,000.
For each, beside ppf_noise_fit_rows: ppf_noise_rows (the "PS" estimator: the
transform alone) on the same rows, and ppf_find_kc_rows on the rows' power
spectra with fn = exp_dc (the search alone) and fn = half_tri (the same
search with the exponential replaced by one division and a compare).  The
difference of the last two over the ppf_noise_fit_rows time is recorded as
exp_share: the part of the call that the 20 n exponentials cost beyond a
cheap basis function.

The device time is Engine.kernel_time("noise") under Engine.set_timing (HIP
events around every launch; all four entry points are timed under that id),
the best of three calls after a warm-up.  --ref also times the numpy
restatement of the same search (tests/noise_fit_reference.py, term by term,
one core) on the 64 x 2048 rows; that restatement, not the reference's
Python 2 with scipy.optimize.brute, is the CPU yardstick.

    python tools/time_noise_fit.py [--ref] [--out profiles/noise_fit_times.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CHUNK = 64000


def make_rows(nrow, nbin, seed, device):
    import torch
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    ph = (torch.arange(nbin, dtype=torch.float64, device=device) + 0.5) / nbin
    sig = 0.02 / (2.0 * np.sqrt(2.0 * np.log(2.0)))
    pulse = 30.0 * torch.exp(-0.5 * ((ph - 0.5) / sig) ** 2)
    return pulse[None] + torch.randn((nrow, nbin), dtype=torch.float64, device=device,
                                     generator=g)


def device_ms(eng, call, reps=3):
    call()  # warm-up: twiddle table, allocations
    best = None
    for _ in range(reps):
        eng.set_timing(True)
        eng.reset_kernel_times()
        call()
        eng.synchronize()
        ms, _ = eng.kernel_time("noise")
        eng.set_timing(False)
        best = ms if best is None else min(best, ms)
    return best


def measure(eng, rows):
    import torch
    nbin = rows.shape[1]
    spec = torch.fft.rfft(rows, dim=1)
    pows = (spec.real ** 2 + spec.imag ** 2) / nbin
    return dict(
        noise_fit_ms=device_ms(eng, lambda: eng.noise_fit_rows(rows)),
        noise_ps_ms=device_ms(eng, lambda: eng.noise_rows(rows)),
        find_kc_exp_dc_ms=device_ms(eng, lambda: eng.find_kc_rows(pows)),
        find_kc_half_tri_ms=device_ms(eng, lambda: eng.find_kc_rows(pows, fn="half_tri")))


def finish(rec):
    rec["exp_share"] = (rec["find_kc_exp_dc_ms"] - rec["find_kc_half_tri_ms"]) / rec["noise_fit_ms"]
    rec["us_per_row"] = 1e3 * rec["noise_fit_ms"] / rec["nrow"]
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", action="store_true", help="also time the numpy restatement")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from pulseportraiture_amd.engine import get_engine
    eng = get_engine(0)
    results = []
    first = None
    for nrow, nbin in ((64, 2048), (512, 1024)):
        rows = make_rows(nrow, nbin, 1, eng.device)
        rec = finish(dict(workload="%d x %d" % (nrow, nbin), nrow=nrow, nbin=nbin,
                          **measure(eng, rows)))
        print(json.dumps(rec), flush=True)
        results.append(rec)
        if first is None:
            first = rows.cpu().numpy()
    total = dict(noise_fit_ms=0.0, noise_ps_ms=0.0, find_kc_exp_dc_ms=0.0,
                 find_kc_half_tri_ms=0.0)
    nrow = 640000
    for c in range(nrow // CHUNK):
        part = measure(eng, make_rows(CHUNK, 2048, 100 + c, eng.device))
        for k in total:
            total[k] += part[k]
        print("chunk", c, json.dumps(part), flush=True)
    rec = finish(dict(workload="640000 x 2048 in chunks of %d" % CHUNK, nrow=nrow, nbin=2048,
                      **total))
    print(json.dumps(rec), flush=True)
    results.append(rec)
    if args.ref:
        from tests import noise_fit_reference as R
        t0 = time.perf_counter()
        for row in first:
            R.get_noise_fit(row)
        rec = dict(workload="64 x 2048", numpy_restatement_one_core_s=time.perf_counter() - t0)
        print(json.dumps(rec), flush=True)
        results.append(rec)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
