#!/usr/bin/env python3
"""Time Engine.scrunch_subints from 16-bit samples against the same result
composed from the kernels the package had before it.

    python tools/time_scrunch.py [--reps 7] [--out profiles/scrunch_times.json] [--small]

Workload: 64 subints x 4 polarisations x 4096 channels x 1024 bins of int16
samples (2 GiB), every polarisation kept, to 64 channels x 512 bins (f = 64,
b = 2), random phases and weights.  One process; the samples are made on the
device and stay there.  The two paths:
  (raw)      eng.scrunch_subints(RawSubints(...), w, phase, 64, 2, all_pols=True)
  (composed) eng.unpack_subints -> eng.rotate_fscrunch on the units
             [nsub npol ngroup, f, nbin] with the weights and phases laid out
             per unit -> / W -> mean of adjacent bins (torch)
After a warm-up of both they alternate, --reps times each, timed with device
events on the engine's stream around the whole path; median, min and max are
recorded.  The two outputs are compared in the same run (the composed path
divides and averages in torch, in another order: agreement to rounding, not
bitwise).

Peak extra device memory, per path, measured before the timing: the rise of
torch's peak allocation over what is allocated when the path starts (inputs
excluded, the path's own output included), plus the growth of the library's
own workspace, read as the fall of the device's free memory that torch's
reserved pool does not account for.  The raw path is measured first, so the
workspace it grows is not counted against the composed path again; the
composed path's figure is therefore a lower bound on a fresh process's.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(v):
    v = [float(x) for x in v]
    return {"median": float(np.median(v)), "min": min(v), "max": max(v), "n": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scrunch_times.json"))
    ap.add_argument("--small", action="store_true", help="8 x 4 x 512 x 1024: a quick check")
    args = ap.parse_args()
    import torch
    from pulseportraiture_amd.engine import RawSubints, get_engine
    eng = get_engine(0)
    dev = eng.device
    nsub, npol, nchan, nbin = (8, 4, 512, 1024) if args.small else (64, 4, 4096, 1024)
    f, b = nchan // 64, 2
    ng, nbo = nchan // f, nbin // b
    g = torch.Generator(device=dev)
    g.manual_seed(20240917)
    raw = torch.empty((nsub, npol, nchan, nbin), dtype=torch.int16, device=dev)
    for s in range(nsub):  # a subint at a time: no wider temporary than one subint
        raw[s] = torch.randint(-32767, 32768, (npol, nchan, nbin), generator=g, device=dev,
                               dtype=torch.int32).to(torch.int16)
    scl = torch.rand((nsub, npol, nchan), generator=g, device=dev, dtype=torch.float64) + 0.5
    offs = torch.randn((nsub, npol, nchan), generator=g, device=dev, dtype=torch.float64)
    w = torch.rand((nsub, nchan), generator=g, device=dev, dtype=torch.float64) + 0.5
    w[:, 7] = 0.0
    ph = torch.rand((nsub, nchan), generator=g, device=dev, dtype=torch.float64) - 0.5
    rs = RawSubints(raw, scl, offs, pmode=0)
    # the composed path's per-unit weights and phases (small: nunit x f)
    wx = w.reshape(nsub, 1, ng, f).expand(nsub, npol, ng, f).reshape(-1, f).contiguous()
    phx = ph.reshape(nsub, 1, ng, f).expand(nsub, npol, ng, f).reshape(-1, f).contiguous()
    W = wx.sum(dim=1)

    def path_raw():
        return eng.scrunch_subints(rs, w, ph, f, b, all_pols=True)[0]

    def path_composed():
        x = eng.unpack_subints(raw, scl, offs, 0)
        prof = eng.rotate_fscrunch(x.reshape(nsub * npol * ng, f, nbin), phx, wx)
        del x
        prof = prof / W[:, None]
        return prof.reshape(nsub, npol, ng, nbo, b).mean(dim=-1)

    def memory(call):
        eng.synchronize()
        torch.cuda.synchronize(dev)
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats(dev)
        alloc0, res0 = torch.cuda.memory_allocated(dev), torch.cuda.memory_reserved(dev)
        free0 = torch.cuda.mem_get_info(dev)[0]
        out = call()
        eng.synchronize()
        torch.cuda.synchronize(dev)
        peak = torch.cuda.max_memory_allocated(dev) - alloc0
        res1 = torch.cuda.memory_reserved(dev)
        free1 = torch.cuda.mem_get_info(dev)[0]
        lib = max(0, (free0 - free1) - (res1 - res0))
        del out
        return {"torch_peak_bytes": int(peak), "library_workspace_growth_bytes": int(lib),
                "peak_extra_bytes": int(peak + lib)}

    mem = {"raw": memory(path_raw), "composed": memory(path_composed)}
    a, c = path_raw(), path_composed()  # warm-up of both
    eng.synchronize()
    diff = float((a - c).abs().max() / c.abs().max())
    del a, c
    st = eng.stream

    def timed(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        out = call()
        e1.record(st)
        e1.synchronize()
        del out
        return e0.elapsed_time(e1)

    ms = {"raw": [], "composed": []}
    for _ in range(args.reps):
        ms["raw"].append(timed(path_raw))
        ms["composed"].append(timed(path_composed))
    r, c = stats(ms["raw"]), stats(ms["composed"])
    nsamp = nsub * npol * nchan * nbin
    rec = {
        "workload": "scrunch %d x %d x %d x %d int16 -> %d channels x %d bins" % (
            nsub, npol, nchan, nbin, ng, nbo),
        "shape": [nsub, npol, nchan, nbin], "f": f, "b": b,
        "method": "one process; both paths warmed up, then alternated %d times each; device "
                  "events on the engine's stream around the whole path; median with min and max. "
                  "Memory: rise of torch's peak allocation over the path's start plus the "
                  "library workspace's growth (fall of free device memory beyond torch's "
                  "reserved pool), raw path first" % args.reps,
        "device_ms": {"raw_scrunch_subints": r, "composed_unpack_fscrunch_divide_mean": c,
                      "composed_over_raw": c["median"] / r["median"]},
        "peak_extra_device_memory": mem,
        "bytes": {"int16_samples": 2 * nsamp, "fp64_copy_the_composed_path_makes": 8 * nsamp,
                  "output": 8 * nsub * npol * ng * nbo},
        "max_rel_difference_raw_vs_composed": diff,
        "device": torch.cuda.get_device_name(dev),
    }
    print(json.dumps(rec, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
