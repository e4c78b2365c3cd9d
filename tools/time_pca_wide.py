"""Time the PCA of wide portraits: the Gram path (ppf_pca_gram_portraits) at
3,328 x 1,024, 4,096 x 2,048 and 16,384 x 2,048, both paths at 2,048 x 512,
and the host yardstick -- np.cov + np.linalg.eigh, what the reference runs --
at 4,096 x 2,048.

Device time is measured with HIP events around the launches (Engine.set_timing)
and split by Engine.pca_gram_times into the mean pass, the Gram tiles, the sum
over slabs, the Jacobi on G and the emit; the second of two calls is reported
(the first allocates the workspace).  The Gram tiles' rate counts the
multiply-adds of the lower triangle, nchan nbin (nbin + 1) flops, and is set
beside the 78.6 TFLOP/s fp64 matrix peak.

    python tools/time_pca_wide.py [--out profiles/pca_wide_times.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_TFLOPS = 78.6


def port_of(nchan, nbin, seed, noise=0.05):
    rng = np.random.default_rng(seed)
    ph = (np.arange(nbin) + 0.5) / nbin
    f = np.linspace(0, 1, nchan)[:, None]
    p = np.exp(-0.5 * ((ph - 0.45 - 0.05 * f) / (0.04 + 0.03 * f)) ** 2) * (1 + 0.5 * f) \
        + 0.4 * np.exp(-0.5 * ((ph - 0.6 + 0.03 * f ** 2) / 0.03) ** 2)
    return p + noise * rng.standard_normal((nchan, nbin)), rng.uniform(0.5, 2.0, nchan)


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from pulseportraiture_amd.engine import get_engine
    eng = get_engine(0)
    results = []
    for nchan, nbin, methods in ((3328, 1024, ("gram",)), (4096, 2048, ("gram",)),
                                 (16384, 2048, ("gram",)), (2048, 512, ("gram", "rows"))):
        port, w = port_of(nchan, nbin, nchan + nbin)
        x = torch.as_tensor(port, device=eng.device)
        wt = torch.as_tensor(w, device=eng.device)
        lam = {}
        for method in methods:
            for rep in range(2):
                eng.set_timing(True)
                eng.reset_kernel_times()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = eng.pca_portraits(x, wt, None, method)
                torch.cuda.synchronize()
                wall = time.perf_counter() - t0
                ms, launches = eng.kernel_time("pca")
                split = eng.pca_gram_times()
                eng.set_timing(False)
            lam[method] = out[1].cpu().numpy()
            rec = dict(shape="%dx%d" % (nchan, nbin), nchan=nchan, nbin=nbin, method=method,
                       device_ms=ms, launches=int(launches), wall_s=wall,
                       sweeps=int(out[3][0]), converged=int(out[3][1]))
            if method == "gram":
                mean_ms, tiles_ms, sum_ms, jacobi_ms, emit_ms = split
                tflops = nchan * nbin * (nbin + 1.0) / (tiles_ms * 1e-3) / 1e12
                rec.update(mean_ms=mean_ms, gram_tiles_ms=tiles_ms, gram_sum_ms=sum_ms,
                           jacobi_ms=jacobi_ms, emit_ms=emit_ms, gram_tiles_tflops=tflops,
                           gram_tiles_peak_fraction=tflops / PEAK_TFLOPS)
            print(json.dumps(rec))
            results.append(rec)
        if len(lam) == 2:
            d = float(np.max(np.abs(lam["gram"][:10] - lam["rows"][:10])) / lam["rows"][0])
            results.append(dict(shape="%dx%d" % (nchan, nbin), gram_vs_rows_dlambda_rel=d))
        if (nchan, nbin) == (4096, 2048):
            t0 = time.perf_counter()
            mean = (port.T * w).T.sum(axis=0) / w.sum()
            ref = np.linalg.eigh(np.cov((port - mean).T, aweights=w, ddof=1))[0][::-1]
            rec = dict(shape="%dx%d" % (nchan, nbin), method="numpy cov + eigh (host)",
                       host_s=time.perf_counter() - t0,
                       dlambda_rel=float(np.max(np.abs(lam["gram"][:10] - ref[:10])) / ref[0]))
            print(json.dumps(rec))
            results.append(rec)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
