"""Time the fits across channels (ppf_powlaw_fit_rows, ppf_line_fit_rows;
ppfit_chanfit.hip).

Shapes: 1 x 64, 1,000 x 64, 100,000 x 64 and 1,000 x 4,096 (rows x points).
Power-law rows: sorted uniform frequencies in [700, 2300] MHz, nu_ref 1500,
A in [0.5, 20], index -4.4 .. 2, S/N 50 per point, a tenth of the points left
out; the fit starts from [1, 0] with leastsq's default tolerances.  Line rows:
y = Dconst dDM nu^-2 + offset + noise over [1100, 1900] MHz with w = errs^-2.
Inputs are on the device before the clock starts.

Per shape and kernel: device time between two events around `calls`
back-to-back calls (enough of them to fill at least a few milliseconds),
divided by `calls`; warm, the median (and the spread) of `reps` such windows.
Beside them, for 1,000 x 64 on one core: the wall time of a loop of
scipy.optimize.leastsq (the reference's configuration: forward differences,
default tolerances) and of a loop of np.polyfit(cov=True).

    python tools/time_chanfit.py [--out profiles/chanfit_times.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(1, 64), (1000, 64), (100000, 64), (1000, 4096)]
Dconst = 0.000241 ** -1


def powlaw_rows(nrow, n, seed):
    rng = np.random.default_rng(seed)
    f = np.sort(rng.uniform(700.0, 2300.0, (nrow, n)), axis=1)
    A = rng.uniform(0.5, 20.0, nrow)[:, None]
    al = rng.uniform(-4.4, 2.0, nrow)[:, None]
    e = A / 50.0 * rng.uniform(0.5, 2.0, (nrow, n))
    y = A * (f / 1500.0) ** al + e * rng.standard_normal((nrow, n))
    e[rng.random((nrow, n)) < 0.1] = 0.0
    return y, e, f


def line_rows(nrow, n, seed):
    rng = np.random.default_rng(seed)
    nu = np.tile(np.linspace(1100.0, 1900.0, n), (nrow, 1))
    e = rng.uniform(0.5e-6, 4e-6, (nrow, n))
    y = (Dconst * rng.uniform(-2e-3, 2e-3, (nrow, 1)) * nu ** -2 +
         rng.uniform(-1e-5, 1e-5, (nrow, 1)) + e * rng.standard_normal((nrow, n)))
    w = e ** -2
    w[rng.random((nrow, n)) < 0.1] = 0.0
    return nu ** -2, y, w


def device_ms(eng, call, reps=15, floor_ms=5.0):
    """(median ms per call, min, max, calls per window) over reps windows."""
    import torch
    for _ in range(3):
        call()
    eng.synchronize()

    def window(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(eng.stream)
        for _ in range(calls):
            call()
        b.record(eng.stream)
        torch.cuda.synchronize()
        return a.elapsed_time(b) / calls
    calls = 1
    while window(calls) * calls < floor_ms and calls < 4096:
        calls *= 2
    ms = sorted(window(calls) for _ in range(reps))
    return ms[len(ms) // 2], ms[0], ms[-1], calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from scipy.optimize import leastsq
    from pulseportraiture_amd.engine import get_engine
    eng = get_engine(0)
    dev = lambda a: torch.as_tensor(a, device=eng.device)
    results = []
    host = {}
    for nrow, n in SHAPES:
        y, e, f = powlaw_rows(nrow, n, 100 + n)
        x, ly, w = line_rows(nrow, n, 200 + n)
        if (nrow, n) == (1000, 64):
            host = dict(y=y, e=e, f=f, x=x, ly=ly, w=w)
        ty, te, tf = dev(y), dev(e), dev(f)
        nu, init = dev(np.full(nrow, 1500.0)), dev(np.tile([1.0, 0.0], (nrow, 1)))
        tx, tly, tw = dev(x), dev(ly), dev(w)
        out, info = eng.powlaw_fit_rows(ty, te, tf, nu, init)
        info = info.cpu().numpy()
        med, lo, hi, calls = device_ms(eng, lambda: eng.powlaw_fit_rows(ty, te, tf, nu, init))
        rec = dict(kernel="ppf_powlaw_fit_rows", nrow=nrow, n=n, device_ms_median=med,
                   device_ms_min=lo, device_ms_max=hi, calls_per_window=calls, windows=15,
                   us_per_row=1e3 * med / nrow, nfev_mean=float(info[:, 1].mean()),
                   nfev_max=int(info[:, 1].max()),
                   status_counts={str(k): int((info[:, 0] == k).sum())
                                  for k in np.unique(info[:, 0])})
        print(json.dumps(rec), flush=True)
        results.append(rec)
        med, lo, hi, calls = device_ms(eng, lambda: eng.line_fit_rows(tx, tly, tw))
        rec = dict(kernel="ppf_line_fit_rows", nrow=nrow, n=n, device_ms_median=med,
                   device_ms_min=lo, device_ms_max=hi, calls_per_window=calls, windows=15,
                   us_per_row=1e3 * med / nrow)
        print(json.dumps(rec), flush=True)
        results.append(rec)

    # the host loops the device calls stand in for, 1,000 x 64 on one core
    def resid(p, y, e, f):
        return (y - p[0] * (f / 1500.0) ** p[1]) / e
    t0 = time.perf_counter()
    for y, e, f in zip(host["y"], host["e"], host["f"]):
        ok = e > 0.0
        leastsq(resid, [1.0, 0.0], args=(y[ok], e[ok], f[ok]), full_output=True)
    t_lsq = time.perf_counter() - t0
    t0 = time.perf_counter()
    for x, y, w in zip(host["x"], host["ly"], host["w"]):
        ok = w > 0.0
        np.polyfit(x[ok], y[ok], 1, w=w[ok], cov=True)
    t_poly = time.perf_counter() - t0
    rec = dict(host_loops="1000 x 64, one core", leastsq_loop_wall_s=t_lsq,
               polyfit_loop_wall_s=t_poly)
    print(json.dumps(rec), flush=True)
    results.append(rec)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(results, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
