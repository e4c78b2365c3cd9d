"""Time the starting template of ppalign on the device.

1. Engine.rotate_fscrunch (ppfit_fscrunch.hip) at 4096 x 256 x 2048 (ppalign's
   config-5 shape) and at 64 x 64 x 2048, beside the composition the package
   offered before it for the same result: Engine.rotate_rows into a new tensor,
   then a weighted sum over channels (torch.einsum, a batched fp64 GEMV).  Both
   are timed with device events around the whole call, alternating, after a
   warm-up call of each; the fused call's own kernel time (Engine.kernel_time
   ("fscrunch"), HIP events around every launch) is taken in a further call.
   The fused kernel reads the data once: its bytes are nunit nchan nbin 8 plus
   the partial spectra and the profiles, over the device time, against the
   HBM peak (8.0 TB/s spec; 6.29 TB/s is what a plain copy reaches).
   --ab-lib PATH times the same calls in a child process that loads another
   build of libppfit.so (tools/build_variant.py), for an A/B of two kernels.
2. The wall time of ppalign.add_archives(palign=True) over 4096 registered
   single-subint archives of that shape, beside one align_archives iteration
   over the same archives (bench.py's ppalign leg).

    python tools/time_add_archives.py [--narch 4096] [--ab-lib PATH] \
        [--out profiles/add_archives_times.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NCHAN, NBIN = 256, 2048
HBM_SPEC_GBS, HBM_COPY_GBS = 8000.0, 6290.0
SLICE = 32  # kFsSlice


def event_ms(torch, call):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = call()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def time_fscrunch(eng, nunit, nchan, nbin, reps=5):
    import torch
    from pulseportraiture_amd import synth
    w = synth.make_workload(nunit, nchan, nbin, seed=777)
    data = eng.synth(w.template, w.phase, w.sigma, w.seed, sub0=w.sub0)
    g = torch.Generator(device="cuda").manual_seed(5)
    ph = torch.rand((nunit, nchan), generator=g, device="cuda", dtype=torch.float64) * 4.0 - 2.0
    wt = torch.rand((nunit, nchan), generator=g, device="cuda", dtype=torch.float64) + 0.5
    torch.cuda.synchronize()

    def fused():
        return eng.rotate_fscrunch(data, ph, wt)

    def composed():
        return torch.einsum("uc,ucb->ub", wt, eng.rotate_rows(data, ph))
    a, b = fused(), composed()  # warm-up: workspaces, the allocator, rocBLAS
    err = float((a - b).abs().max() / b.abs().max())
    del a, b
    tf, tc = [], []
    for _ in range(reps):  # alternating
        tf.append(event_ms(torch, fused)[0])
        tc.append(event_ms(torch, composed)[0])
    eng.set_timing(True)
    eng.reset_kernel_times()
    fused()
    kms, launches = eng.kernel_time("fscrunch")
    eng.set_timing(False)
    nslice = (nchan + SLICE - 1) // SLICE
    nh = nbin // 2 + 1
    nbytes = nunit * nchan * nbin * 8 + 2 * nunit * (nslice + 1) * nh * 16 + nunit * nbin * 8
    best = min(tf)
    rec = dict(shape=[nunit, nchan, nbin], fused_ms=[round(t, 3) for t in tf],
               composed_ms=[round(t, 3) for t in tc], fused_best_ms=round(best, 3),
               composed_best_ms=round(min(tc), 3), speedup=round(min(tc) / best, 2),
               fused_kernel_ms=round(kms, 3), fused_launches=int(launches),
               fused_bytes=nbytes, fused_GBs=round(nbytes / best / 1e6, 1),
               hbm_fraction_of_spec=round(nbytes / best / 1e6 / HBM_SPEC_GBS, 3),
               hbm_fraction_of_copy=round(nbytes / best / 1e6 / HBM_COPY_GBS, 3),
               max_rel_diff_fused_vs_composed=err,
               lib=os.path.basename(os.environ.get("PPF_LIB", "libppfit.so")))
    del data
    torch.cuda.empty_cache()
    return rec


def time_add_archives(eng, narch):
    import torch
    from pulseportraiture_amd import archive, ppalign, synth
    w = synth.make_workload(narch, NCHAN, NBIN, seed=555 + 5)
    data = eng.synth(w.template, w.phase, w.sigma, w.seed, sub0=w.sub0)
    torch.cuda.synchronize()
    names = ["time_aa_%d" % i for i in range(narch)]
    archive.register_archives(names, [dict(subints=data[i:i + 1, None], freqs=w.freqs, Ps=[w.P],
                                           epochs=[(57000 + i, 0, 0.0)], DM=w.DM0)
                                      for i in range(narch)])
    archive.register_archive("time_aa_guess", dict(subints=w.model[None, None], freqs=w.freqs,
                                                   Ps=[w.P], epochs=[(57000, 0, 0.0)],
                                                   DM=w.DM0, dmc=1))

    def wall(call):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = call()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    def add():
        return ppalign.add_archives(names, None, palign=True, quiet=True)

    def align():
        return ppalign.align_archives(names, "time_aa_guess", fit_dm=True, niter=1, quiet=True)
    add(), align()  # warm-up
    ta, tl = [], []
    for _ in range(2):
        ta.append(wall(add)[0])
        tl.append(wall(align)[0])
    # the device's share of add_archives: its kernels' own time
    eng.set_timing(True)
    eng.reset_kernel_times()
    add()
    kt = {k: round(eng.kernel_time(k)[0], 3) for k in ("fscrunch", "phase_shift", "rot_accum",
                                                       "irfft")}
    eng.set_timing(False)
    for nm in names + ["time_aa_guess"]:
        archive.unregister_archive(nm)
    return dict(workload="add_archives(palign=True) beside one align_archives iteration",
                shape=[narch, NCHAN, NBIN], add_archives_wall_s=[round(t, 4) for t in ta],
                align_archives_1iter_wall_s=[round(t, 4) for t in tl],
                add_over_align=round(min(ta) / min(tl), 2), add_archives_kernel_ms=kt)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--narch", type=int, default=4096)
    ap.add_argument("--ab-lib", default=None, help="another build of libppfit.so to time beside")
    ap.add_argument("--only-fscrunch", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from pulseportraiture_amd.engine import get_engine
    eng = get_engine(0)
    results = []
    for shape in ((args.narch, NCHAN, NBIN), (64, 64, NBIN)):
        rec = dict(workload="rotate_fscrunch", **time_fscrunch(eng, *shape))
        print(json.dumps(rec), flush=True)
        results.append(rec)
    if args.ab_lib:
        # a fresh process: the library is chosen when it is first loaded
        env = dict(os.environ, PPF_LIB=os.path.abspath(args.ab_lib))
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--only-fscrunch",
                              "--narch", str(args.narch)], env=env, check=True,
                             stdout=subprocess.PIPE, text=True).stdout
        for line in out.splitlines():
            if line.startswith("{"):
                rec = json.loads(line)
                rec["workload"] = "rotate_fscrunch (A/B library)"
                print(json.dumps(rec), flush=True)
                results.append(rec)
    if not args.only_fscrunch:
        rec = time_add_archives(eng, args.narch)
        print(json.dumps(rec), flush=True)
        results.append(rec)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
