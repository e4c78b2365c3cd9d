"""Time the two ways of making 16-bit fake-pulsar samples on the device.

ppf_fake_subints with packed output runs, for a power-of-two nbin, one kernel
that makes each row in LDS and stores only its int16 samples ("fused"); the
alternative is the fp64 generator followed by ppf_pack_subints ("two_kernel"),
which moves the fp64 rows through HBM (8 B written, 8 B read, 2 B written per
sample against 2 B).  Both give the same bytes (tests/test_gpu_fake_pulsar.py).
The two are timed alternately at one shape: wall time of the calls (each ends
in the stream wait that returns the pack status) and the device time of their
kernels (HIP events, Engine.set_timing) in a second pass.

    python tools/time_fake_pulsar.py [--nsub 2000] [--out profiles/fake_pulsar_times.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nsub", type=int, default=2000)
    ap.add_argument("--nchan", type=int, default=64)
    ap.add_argument("--nbin", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from pulseportraiture_amd import synth
    from pulseportraiture_amd.engine import get_engine
    eng = get_engine(0)
    w = synth.make_workload(args.nsub, args.nchan, args.nbin)
    model = torch.as_tensor(w.template, device=eng.device)
    phase = torch.as_tensor(w.phase, device=eng.device)
    amp = torch.ones((args.nsub, args.nchan), dtype=torch.float64, device=eng.device)
    sigma = torch.full((args.nchan,), w.sigma, dtype=torch.float64, device=eng.device)

    def fused():
        return eng.fake_subints(model, phase, amp, sigma, w.seed, packed=True)

    def two_kernel():
        return eng.pack_subints(eng.fake_subints(model, phase, amp, sigma, w.seed))

    paths = (("fused", fused), ("two_kernel", two_kernel))
    outs = {k: fn() for k, fn in paths}  # warm-up: tables, workspace, allocator
    same = all(torch.equal(a, b) for a, b in zip(outs["fused"], outs["two_kernel"]))
    del outs
    wall = {k: [] for k, _ in paths}
    for _ in range(args.reps):  # alternate, so drift reaches both alike
        for k, fn in paths:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            wall[k].append(time.perf_counter() - t0)
    dev = {}
    eng.set_timing(True)
    for k, fn in paths:
        eng._chk(eng.lib.ppf_reset_kernel_times(eng.ctx))
        for _ in range(args.reps):
            fn()
        dev[k] = {kid: eng.kernel_time(kid)[0] / args.reps for kid in ("synth", "pack")}
    eng.set_timing(False)
    nsamp = args.nsub * args.nchan * args.nbin
    rec = dict(nsub=args.nsub, npol=1, nchan=args.nchan, nbin=args.nbin, reps=args.reps,
               samples=nsamp, outputs_equal=bool(same),
               hbm_bytes_per_sample=dict(fused=2, two_kernel=18),
               wall_ms={k: dict(median=1e3 * float(np.median(v)), min=1e3 * float(np.min(v)),
                                max=1e3 * float(np.max(v))) for k, v in wall.items()},
               device_ms=dev)
    rec["fused_over_two_kernel_wall"] = rec["wall_ms"]["fused"]["median"] / \
        rec["wall_ms"]["two_kernel"]["median"]
    print(json.dumps(rec))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
