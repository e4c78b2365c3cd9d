#!/usr/bin/env python3
"""Time the mixed-radix row FFT (RowSmooth, option row_fft) against another
build of libppfit.so -- the parent commit's -- and against its own direct-sum
path (row_fft 0).

    python tools/time_row_fft.py [--ab-lib PARENT.so] [--rounds 3]
                                 [--out profiles/row_fft_times.json]

Every measurement runs in a fresh process (the library is chosen when it is
first loaded, PPF_LIB), the variants alternating within each round: parent,
new with row_fft 0, new with row_fft 1.  Inputs are made on the device from a
seed.  Per variant and nbin in (1000, 1536, 2000, 3000, 8000), 2,000 x 64
rows, HIP-event time of the launch brackets (Engine.set_timing), best of
three calls after a warm-up:
  noise       ppf_noise_rows: k_noise_rows, the forward transform and a power sum
  rfft_irfft  ppf_instrumental_response_rows with no response: k_rfft_rows,
              a pointwise kernel and k_irfft_rows
  rotate      ppf_rotate_rows: k_rotate_rows, forward and back in one kernel
  data_pass   the fit's data pass (id data_xspec) of fit_batch, phi + DM
  fit_ms      wall time of that fit_batch, as bench.py --full's generic_nbin leg
and ppalign's rotate-and-sum (k_rot_accum) at 512 x 256 x 2000.  The fit at
nbin 2048 (same batch) is timed beside, for the ratio the leg reports.

--check: instead of times, every variant dumps the bytes of the row entry
points and of a phi + DM fit at seven nbin; the parent and the new library
under row_fft 0 must agree byte for byte at every length, and the new library
under row_fft 1 at the powers of two.

The verdict per shape and leg: the new path's range over the rounds lies
below the parent's range (true / false).
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NSUB, NCHAN = 2000, 64
NBINS = (1000, 1536, 2000, 3000, 8000)
ALIGN = (512, 256, 2000)
CHECK_NBINS = (96, 100, 128, 1000, 1536, 2048, 8100)
LEGS = ("noise", "rfft_irfft", "rotate", "data_pass", "fit_ms")


def engine(row_fft):
    """The engine of the library PPF_LIB names; a build from before the
    option and ppf_row_transform (the parent's) is used as it is."""
    import ctypes
    import torch  # noqa: F401  (before the library: it brings its own HIP runtime)
    from pulseportraiture_amd import _lib
    path = os.environ.get("PPF_LIB") or _lib.LIB_PATH
    old = not hasattr(ctypes.CDLL(path), "ppf_row_transform")
    if old:
        _lib.EXPORTS.pop("ppf_row_transform")
    from pulseportraiture_amd.engine import Engine
    eng = Engine(0)
    if not old:
        eng.set_option("row_fft", row_fft)
    elif row_fft is not None and row_fft != 0:
        raise SystemExit("this library has no row_fft option")
    return eng


def event_ms(eng, kid, call, reps=3):
    call()  # warm-up: twiddle table, allocations
    best = None
    for _ in range(reps):
        eng.set_timing(True)
        eng.reset_kernel_times()
        call()
        eng.synchronize()
        ms, _ = eng.kernel_time(kid)
        eng.set_timing(False)
        best = ms if best is None else min(best, ms)
    return best


def rows_of(nrow, nbin, seed):
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    ph = (torch.arange(nbin, dtype=torch.float64, device="cuda") + 0.5) / nbin
    pulse = 30.0 * torch.exp(-0.5 * ((ph - 0.5) / 0.01) ** 2)
    return pulse[None] + torch.randn((nrow, nbin), dtype=torch.float64, device="cuda", generator=g)


def time_fit(eng, nbin, seed):
    """(data pass event ms, fit wall ms) of 2,000 x 64 subints, phi + DM."""
    import torch
    from pulseportraiture_amd import synth
    w = synth.make_workload(1, NCHAN, nbin, seed=seed + nbin)
    g = torch.Generator(device="cuda").manual_seed(seed)
    ph = torch.rand(NSUB, 1, generator=g, device="cuda", dtype=torch.float64) * 0.2 - 0.1
    model = torch.as_tensor(w.model, device="cuda")
    data = eng.rotate_rows(model.expand(NSUB, NCHAN, nbin).reshape(-1, nbin).contiguous(),
                           ph.expand(NSUB, NCHAN).reshape(-1)).reshape(NSUB, NCHAN, nbin)
    data += 1.5 * torch.randn(data.shape, generator=g, device="cuda", dtype=torch.float64)
    nu = float(np.mean(w.freqs))

    def fit():
        return eng.fit_batch(data, w.model, w.freqs, w.P, [0.0, w.DM0, 0, 0, 0], [1, 1, 0, 0, 0],
                             nu_fit=[nu] * 3, guess=True)
    dp = event_ms(eng, "data_xspec", fit)
    best = None
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fit()
        torch.cuda.synchronize()
        t = (time.perf_counter() - t0) * 1e3
        best = t if best is None else min(best, t)
    return dp, best


def worker_time(row_fft, seed=20240917):
    import torch
    eng = engine(row_fft)
    out = {}
    for nbin in NBINS:
        rows = rows_of(NSUB * NCHAN, nbin, seed + nbin)
        freqs = np.linspace(1200.0, 1600.0, rows.shape[0])
        ph = torch.linspace(-0.4, 0.4, rows.shape[0], dtype=torch.float64, device="cuda")
        rec = dict(
            noise=event_ms(eng, "noise", lambda: eng.noise_rows(rows)),
            rfft_irfft=event_ms(eng, "model_fft",
                                lambda: eng.instrumental_response_rows(rows, freqs)),
            rotate=event_ms(eng, "rotate", lambda: eng.rotate_rows(rows, ph)))
        del rows, ph
        rec["data_pass"], rec["fit_ms"] = time_fit(eng, nbin, seed)
        out[str(nbin)] = rec
        torch.cuda.empty_cache()
    _, out["fit_ms_2048"] = time_fit(eng, 2048, seed)
    ns, nc, nb = ALIGN
    d = rows_of(ns * nc, nb, seed).reshape(ns, nc, nb)
    ph = torch.linspace(-0.4, 0.4, ns * nc, dtype=torch.float64, device="cuda").reshape(ns, nc)
    wt = torch.ones(ns, nc, dtype=torch.float64, device="cuda")
    acc = torch.zeros(nc, nb // 2 + 1, 2, dtype=torch.float64, device="cuda")
    out["rot_accum_%dx%dx%d" % ALIGN] = event_ms(
        eng, "rot_accum", lambda: eng.rotate_accumulate(d, ph, wt, acc))
    print("RESULT " + json.dumps(out), flush=True)


def worker_check(row_fft, path):
    import torch
    from pulseportraiture_amd import synth
    eng = engine(row_fft)
    store = {}
    for nbin in CHECK_NBINS:
        w = synth.make_workload(3, 6, nbin, seed=900 + nbin)
        data = synth.workload_data_host(w)
        rows, ph = data[0], np.linspace(-0.3, 0.4, 6)
        tau = np.linspace(0.0, 2e-3, 6)
        acc = torch.zeros(6, nbin // 2 + 1, 2, dtype=torch.float64, device=eng.device)
        eng.rotate_accumulate(data, np.stack([ph, -ph, 2 * ph]), np.ones((3, 6)), acc)
        outs = dict(
            noise=eng.noise_rows(rows), irfft=eng.irfft_rows(np.fft.rfft(rows, axis=-1), nbin),
            shift=eng.phase_shift_batch(rows, w.model, model_idx=np.arange(6)),
            chi2=eng.resid_chi2_rows(rows, ph, w.model, np.ones(6), np.ones(6), 100.0, tau=tau),
            rotate=eng.rotate_rows(rows, ph), scatter=eng.scatter_rotate_rows(rows, ph, 100 * tau),
            synth=eng.synth(w.model, np.stack([ph, -ph]), 1.5, 77), noise_fit=eng.noise_fit_rows(rows),
            accum=acc)
        fit = eng.fit_batch(data, w.model, w.freqs, w.P, [0.0, w.DM0, 0, 0, 0], [1, 1, 0, 0, 0],
                            nu_fit=[float(np.mean(w.freqs))] * 3, guess=True)
        outs.update({"fit_" + k: v for k, v in fit.items() if not k.startswith("_")})
        for k, v in outs.items():
            store["%s@%d" % (k, nbin)] = v.detach().cpu().numpy()
    np.savez(path, **store)


def child(mode, lib, row_fft, extra=()):
    env = dict(os.environ)
    if lib:
        env["PPF_LIB"] = os.path.abspath(lib)
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", mode, "--row-fft", str(row_fft)]
    res = subprocess.run(cmd + list(extra), env=env, check=True, stdout=subprocess.PIPE, text=True)
    for line in res.stdout.splitlines():
        if line.startswith("RESULT "):
            return json.loads(line[7:])
    return None


def spread(vals):
    return [round(min(vals), 4), round(max(vals), 4)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ab-lib", default=None, help="the parent commit's libppfit.so")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--worker", default=None)
    ap.add_argument("--row-fft", type=int, default=1)
    ap.add_argument("--dump", default=None)
    args = ap.parse_args()
    if args.worker == "time":
        return worker_time(args.row_fft)
    if args.worker == "check":
        return worker_check(args.row_fft, args.dump)

    variants = [("new_row_fft_0", None, 0), ("new_row_fft_1", None, 1)]
    if args.ab_lib:
        variants.insert(0, ("parent", args.ab_lib, 0))
    if args.check:
        import tempfile
        rec = {}
        with tempfile.TemporaryDirectory() as d:
            for name, lib, rf in variants:
                child("check", lib, rf, ["--dump", os.path.join(d, name + ".npz")])
            z = {name: np.load(os.path.join(d, name + ".npz")) for name, _, _ in variants}
            base = z["parent"] if args.ab_lib else z["new_row_fft_0"]
            for name in ("new_row_fft_0", "new_row_fft_1"):
                for nbin in CHECK_NBINS:
                    keys = [k for k in base.files if k.endswith("@%d" % nbin)]
                    same = all(np.array_equal(base[k], z[name][k], equal_nan=True) for k in keys)
                    rec.setdefault(name, {})[str(nbin)] = bool(same)
        rec["against"] = "parent" if args.ab_lib else "new_row_fft_0"
        print(json.dumps(rec, indent=1))
        result = {"byte_identical": rec}
    else:
        runs = {name: [] for name, _, _ in variants}
        for _ in range(args.rounds):
            for name, lib, rf in variants:
                runs[name].append(child("time", lib, rf))
                print(name, json.dumps(runs[name][-1]), flush=True)
        result = {"shape": [NSUB, NCHAN], "rounds": args.rounds, "unit": "ms", "ranges": {},
                  "new_below_parent": {}}
        base = "parent" if args.ab_lib else "new_row_fft_0"
        result["against"] = base
        flat = lambda r: dict([("%s@%s" % (leg, nb), r[nb][leg]) for nb in map(str, NBINS)  # noqa: E731
                               for leg in LEGS] +
                              [(k, v) for k, v in r.items() if not isinstance(v, dict)])
        for name in runs:
            rows = [flat(r) for r in runs[name]]
            result["ranges"][name] = {k: spread([r[k] for r in rows]) for k in rows[0]}
        for k, new in result["ranges"]["new_row_fft_1"].items():
            result["new_below_parent"][k] = bool(new[1] < result["ranges"][base][k][0])
        print(json.dumps(result["new_below_parent"], indent=1))
    if args.out:
        old = {}
        if os.path.exists(args.out):
            with open(args.out) as f:
                old = json.load(f)
        old.update(result)
        with open(args.out, "w") as f:
            json.dump(old, f, indent=1)


if __name__ == "__main__":
    main()
